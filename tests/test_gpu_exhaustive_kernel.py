"""ds_exhaustive_fold_device and ds_exhaustive_finish_device through the C ABI, on crafted probabilities, against the NumPy
restatement of the rule (tests/exhaustive_cases.py), bit for bit: every shape folded in 1, 2 and 7 calls, ties across slice
and call boundaries, fewer rows than slots, the level structure of a long tile, the argument errors."""
import numpy as np
import pytest

import exhaustive_cases as ec
from doppel_speller_amd import _lib

pytestmark = pytest.mark.gpu

SLICE_KEYS = 4096              # keys one workgroup of ds_exhaustive_select_kernel holds (kSliceKeys)


def _fold(probabilities, n, calls, row_first=0):
    """The running keys and the finished slots after folding the table in `calls` calls."""
    n_queries, n_rows = probabilities.shape
    running = _lib.DeviceArray.from_host(np.zeros((n_queries, n), dtype=np.uint64))
    for first, last in ec.split(n_rows, calls):
        tile = _lib.DeviceArray.from_host(np.ascontiguousarray(probabilities[:, first:last]))
        _lib.check(_lib.lib().ds_exhaustive_fold_device(tile.ptr, n_queries, last - first, row_first + first, n,
                                                        running.ptr, _lib.pointer(None)), "ds_exhaustive_fold_device")
    outputs = [_lib.DeviceArray((n_queries * n,), dtype) for dtype in (np.int32, np.float32)]
    for out in outputs:                 # a slot the kernel leaves out shows as 0x55 bytes
        _lib.check(_lib.lib().ds_memset(out.ptr, 0x55, out.nbytes, 0), "ds_memset")
    _lib.check(_lib.lib().ds_exhaustive_finish_device(running.ptr, n_queries, n, *(a.ptr for a in outputs),
                                                      _lib.pointer(None)), "ds_exhaustive_finish_device")
    _lib.check(_lib.lib().ds_stream_sync(_lib.pointer(None), 0), "sync")
    return running.to_host(), tuple(a.to_host().reshape(n_queries, n) for a in outputs)


def _marks(n_rows, calls):
    """Rows either side of every call boundary and of every slice boundary inside a call."""
    marks = []
    for first, last in ec.split(n_rows, calls):
        marks += [first - 1, first] + [first + at for at in range(SLICE_KEYS - 1, last - first, SLICE_KEYS)] + \
                 [first + at for at in range(SLICE_KEYS, last - first, SLICE_KEYS)]
    return tuple(marks)


@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 8193])
@pytest.mark.parametrize("n", [1, 5, 64])
@pytest.mark.parametrize("n_queries", [1, 3])
def test_every_shape_in_one_two_and_seven_calls(n_queries, n, n_rows):
    """n = 64 above 1 and 63 rows leaves unfilled slots; "equal" must give the lowest rows; "straddle" puts the one
    maximum either side of every slice and call boundary."""
    for kind in ec.KINDS:
        for calls in (1, 2, 7):
            probabilities = ec.make_probabilities(n_queries, n_rows, kind, seed=n_rows + n, marks=_marks(n_rows, calls))
            keys, slots = _fold(probabilities, n, calls, row_first=0)
            what = (kind, calls)
            assert np.array_equal(keys, ec.best_keys(probabilities, n)), what
            assert ec.same_best(slots, ec.best_rows(probabilities, n)), what
            if kind == "equal":
                assert (slots[0][:, :min(n, n_rows)] == np.arange(min(n, n_rows))).all(), what


def test_rows_that_do_not_start_at_zero_and_a_fold_of_no_rows():
    probabilities = ec.make_probabilities(3, 200, "few", seed=9)
    keys, slots = _fold(probabilities, 5, 2, row_first=2 ** 31 - 200)          # the last rows a key can hold
    assert ec.same_best(slots, ec.best_rows(probabilities, 5, 2 ** 31 - 200))
    assert np.array_equal(keys, ec.best_keys(probabilities, 5, 2 ** 31 - 200))
    running = _lib.DeviceArray.from_host(keys)
    tile = _lib.DeviceArray((1,), np.float32)
    fold = _lib.lib().ds_exhaustive_fold_device
    assert fold(tile.ptr, 3, 0, 0, 5, running.ptr, _lib.pointer(None)) == 0        # no rows: nothing changes
    assert fold(tile.ptr, 0, 10, 0, 5, running.ptr, _lib.pointer(None)) == 0       # no queries
    _lib.check(_lib.lib().ds_stream_sync(_lib.pointer(None), 0), "sync")
    assert np.array_equal(running.to_host(), keys)


@pytest.mark.parametrize("n", [5, 64])
def test_a_tile_long_enough_for_every_level(n):
    """300,000 rows of one query: 74 slices at level 0; at n = 64 their 4,736 keys take two slices at level 1 and a level
    2, at n = 5 level 1 is the last.  Ties everywhere ("few"), and the same table in two calls."""
    probabilities = ec.make_probabilities(1, 300000, "few", seed=n)
    probabilities[0, [299999, 150000, 4095, 4096]] = 0.875
    expected = ec.best_rows(probabilities, n)
    assert expected[0][0, :4].tolist() == [4095, 4096, 150000, 299999]
    for calls in (1, 2):
        keys, slots = _fold(probabilities, n, calls)
        assert ec.same_best(slots, expected), calls
        assert np.array_equal(keys, ec.best_keys(probabilities, n)), calls


def test_argument_errors():
    probabilities = ec.make_probabilities(2, 100, "random", seed=1)
    tile = _lib.DeviceArray.from_host(probabilities)
    before = np.full((2, 5), 7, dtype=np.uint64)
    running = _lib.DeviceArray.from_host(before)
    fold, finish = _lib.lib().ds_exhaustive_fold_device, _lib.lib().ds_exhaustive_finish_device
    good = [tile.ptr, 2, 100, 0, 5, running.ptr, _lib.pointer(None)]
    for position, value in ((0, _lib.pointer(None)), (5, _lib.pointer(None)), (4, 0), (4, 65), (4, -1), (1, -1), (2, -1),
                            (3, -1), (3, 2 ** 31)):
        bad = list(good)
        bad[position] = value
        assert fold(*bad) == -1, (position, value)
        assert _lib.lib().ds_last_error()
    outputs = [_lib.DeviceArray.from_host(np.full(10, 0x55555555, dtype=np.int32)),
               _lib.DeviceArray.from_host(np.full(10, 0x55555555, dtype=np.int32).view(np.float32))]
    good_finish = [running.ptr, 2, 5, outputs[0].ptr, outputs[1].ptr, _lib.pointer(None)]
    for position, value in ((0, _lib.pointer(None)), (3, _lib.pointer(None)), (4, _lib.pointer(None)), (2, 0), (2, 65),
                            (1, -1)):
        bad = list(good_finish)
        bad[position] = value
        assert finish(*bad) == -1, (position, value)
    _lib.check(_lib.lib().ds_stream_sync(_lib.pointer(None), 0), "sync")
    # nothing was launched: the running list and the outputs are as they were
    assert np.array_equal(running.to_host(), before)
    assert (outputs[0].to_host() == 0x55555555).all() and (outputs[1].to_host().view(np.int32) == 0x55555555).all()
    option = _lib.lib().ds_exhaustive_option
    assert option(b"tile_pairs", -1) == -1 and option(b"tile_pairs", 2 ** 24 + 1) == -1
    assert option(b"no_such_option", 1) == -1 and option(None, 1) == -1
    assert option(b"tile_pairs", 0) == 0
    rank = _lib.lib().ds_exhaustive_rank_device
    assert rank(None, None, None, 0, 1, 5, 0, 1, outputs[0].ptr, outputs[1].ptr, _lib.pointer(None)) == -1
