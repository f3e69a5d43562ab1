"""Every process-wide ds_*_option setter, from one table: accepted range, the meaning of 0, and the shared messages.

The library loads without a device and no setter touches one.  ds_forest_option takes a handle that only a device can
make: its ranges are checked by the forest's GPU tests (test_gpu_contributions.py, test_gpu_inspect.py,
test_gpu_refresh.py); here only its null checks."""
import ctypes

import pytest

from doppel_speller_amd import _lib

# (entry point, option, low, high, zero_accepted): include/doppel_amd.h states each range next to its setter
ROWS = [
    ("ds_index_build_option", "duplicate_hash_bits", 0, 64, True),
    ("ds_rank_option", "lds_keys", 0, 512, True),
    ("ds_exhaustive_option", "tile_pairs", 0, 1 << 24, True),
    ("ds_sweep_option", "queries_per_group", 0, 1 << 30, True),
    ("ds_sweep_option", "bootstrap_tile", 0, 64, True),
    ("ds_sweep_option", "bootstrap_max_blocks", 0, 65535, True),
    ("ds_sweep_option", "bootstrap_replicates_per_group", 0, (1 << 16) + 1, True),
    ("ds_duplicates_option", "max_blocks", 0, 1 << 20, True),
    ("ds_assign_option", "max_blocks", 0, 1 << 20, True),
    ("ds_assign_option", "rounds_per_sync", 1, 1024, False),
    ("ds_cuts_option", "column_group", 0, 96, True),
    ("ds_trainer_batch_option", "max_blocks", 0, (1 << 31) - 1, True),
    ("ds_metrics_option", "max_blocks", 0, (1 << 31) - 1, True),
    ("ds_bootstrap_option", "max_blocks", 0, 65535, True),
    ("ds_bootstrap_option", "replicates_per_block", 0, (1 << 16) + 1, True),
    ("ds_bootstrap_option", "table_in_lds", 0, 1, True),
    ("ds_calibrate_option", "max_blocks", 0, 65535, True),
    ("ds_calibrate_option", "segment_points", 2, 2048, True),
    ("ds_edit_option", "pairs_per_group", 0, 16, True),
    ("ds_edit_option", "max_blocks", 0, 65536, True),
    ("ds_hard_option", "max_blocks", 0, 65536, True),
]
# the defaults that are not spelled 0
DEFAULTS = {("ds_rank_option", "lds_keys"): 512, ("ds_assign_option", "rounds_per_sync"): 8,
            ("ds_bootstrap_option", "table_in_lds"): 1}
ENTRIES = sorted({row[0] for row in ROWS})


@pytest.fixture(scope="module")
def library():
    import doppel_speller_amd as ds
    return _lib._declare(ctypes.CDLL(ds.build_library()))


@pytest.mark.parametrize("entry,option,low,high,zero_accepted", ROWS, ids=[f"{row[0]}-{row[1]}" for row in ROWS])
def test_option_range(library, entry, option, low, high, zero_accepted):
    setter, name = getattr(library, entry), option.encode()
    try:
        for value in (low - 1, high + 1):
            assert setter(name, value) == -1, value
            message = library.ds_last_error()
            assert entry.encode() in message and name in message and str(value).encode() in message, message
            assert f"[{low}, {high}]".encode() in message, message
        assert setter(name, low) == 0 and setter(name, high) == 0
        assert setter(name, 0) == (0 if zero_accepted else -1)
        if not zero_accepted:
            assert entry.encode() in library.ds_last_error() and name in library.ds_last_error()
    finally:
        assert setter(name, DEFAULTS.get((entry, option), 0)) == 0


@pytest.mark.parametrize("entry", ENTRIES)
def test_null_and_unknown_names(library, entry):
    setter = getattr(library, entry)
    assert setter(None, 0) == -1
    assert library.ds_last_error() == entry.encode() + b": null name"
    assert setter(b"no_such_option", 0) == -1
    assert library.ds_last_error() == entry.encode() + b": unknown option 'no_such_option'"


def test_forest_option_refuses_null_forest(library):
    assert library.ds_forest_option(None, b"max_blocks", 0) == -1
    assert b"ds_forest_option: null forest" in library.ds_last_error()


def test_every_named_setter_has_a_row(library):
    named = {symbol for symbol in _lib.EXPORTED_SYMBOLS
             if symbol.endswith("_option") and getattr(library, symbol).argtypes[0] is ctypes.c_char_p}
    assert named == set(ENTRIES)
    assert {symbol for symbol in _lib.EXPORTED_SYMBOLS if symbol.endswith("_option")} - named == \
        {"ds_index_option", "ds_titles_option", "ds_forest_option"}


def test_python_set_option_raises_with_the_shared_message(library):
    with pytest.raises(_lib.DoppelError, match=r"ds_edit_option: max_blocks = -1 out of range \[0, 65536\]"):
        _lib.set_option("ds_edit_option", "max_blocks", -1)
    _lib.set_option("ds_edit_option", "max_blocks", 0)
