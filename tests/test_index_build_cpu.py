"""CPU-only checks of the device index build's surface: the `build` / `build_index` keyword is validated before any
library call, the header declares the new entry points, the build compiles the new file, and the NumPy restatement of
the duplicate-rank rule (index_build_cases.duplicate_ranks_rule) agrees with the host's ds_index_duplicate_ranks where
no hashes collide -- which pins the restatement before the GPU tests use it under truncated hashes."""
import ctypes
import os
import re

import numpy as np
import pytest

import index_build_cases as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def no_library(monkeypatch):
    """Any use of the library fails the test: validation has to raise first."""
    from doppel_speller_amd import _lib

    def refuse():
        raise AssertionError("the library was used before the arguments were validated")
    monkeypatch.setattr(_lib, "lib", refuse)


@pytest.mark.parametrize("bad", ["Device", "gpu", "", None, 1, b"host"])
def test_build_keyword_is_validated_before_any_library_call(no_library, bad):
    import doppel_speller_amd as ds
    from doppel_speller_amd.prediction import TruthSide
    from doppel_speller_amd.training_set import FeatureEngineering
    rowptr, idx = np.array([0, 1], dtype=np.int64), np.array([0], dtype=np.int32)
    one = np.ones(1, dtype=np.float32)
    with pytest.raises(ValueError, match="build must be one of"):
        ds.TruthIndex(rowptr, idx, one, one, build=bad)
    with pytest.raises(ValueError, match="build_index must be one of"):
        TruthSide(["some title"], build_index=bad)
    with pytest.raises(ValueError, match="build_index must be one of"):
        ds.Prediction(["some title", "another title"], [0, 1], object(), top_n=1, build_index=bad)
    with pytest.raises(ValueError, match="build_index must be one of"):
        FeatureEngineering(["some title"], [0], ["some title"], [0], top_n=1, sample_n=1, build_index=bad)
    with pytest.raises(ValueError, match="build_index must be one of"):
        ds.train_model(["some title"], [0], ["some title"], [0], top_n=1, sample_n=1, build_index=bad)


def test_header_declares_the_new_entry_points():
    header = open(os.path.join(ROOT, "include", "doppel_amd.h")).read()
    assert re.search(r"int ds_index_create_device\(const int64_t \*rowptr, const int32_t \*truth_idx, const float \*idf32, "
                     r"const float \*sums32,\s+int64_t V, int64_t N, int device, ds_index \*\*out\);", header)
    assert "int ds_index_read(const ds_index *index, const char *name, void *dst, size_t capacity, size_t *bytes);" in header
    assert "int ds_index_build_option(const char *name, int64_t value);" in header


def test_the_build_compiles_the_new_file_and_exports_its_entry_points():
    from doppel_speller_amd import _lib
    assert "ds_index_build.hip" in _lib._SOURCES
    assert os.path.exists(os.path.join(ROOT, "doppel-speller_amd", "csrc", "ds_index_build.hip"))
    assert {"ds_index_create_device", "ds_index_read", "ds_index_build_option"} <= set(_lib.EXPORTED_SYMBOLS)
    library = ctypes.CDLL(_lib.build_library())
    for name in ("ds_index_create_device", "ds_index_read", "ds_index_build_option"):
        assert hasattr(library, name), name
    # argument errors need no GPU: the option's range, and the host's own message for a null input
    library.ds_last_error.restype = ctypes.c_char_p
    assert library.ds_index_build_option(b"duplicate_hash_bits", ctypes.c_int64(65)) == -1
    assert library.ds_index_build_option(b"no_such_option", ctypes.c_int64(0)) == -1
    assert library.ds_index_build_option(b"duplicate_hash_bits", ctypes.c_int64(0)) == 0
    out = ctypes.c_void_p(1)
    assert library.ds_index_create_device(None, None, None, None, ctypes.c_int64(0), ctypes.c_int64(0), 0,
                                          ctypes.byref(out)) == -1
    assert out.value is None and library.ds_last_error().startswith(b"ds_index_create: null input")


def _host_ranks(library, rowptr, truth_idx, sums32, v, n):
    out = np.full(n, 0xffff, dtype=np.uint16)
    pointer = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    assert library.ds_index_duplicate_ranks(pointer(rowptr), pointer(truth_idx), pointer(sums32), ctypes.c_int64(v),
                                            ctypes.c_int64(n), pointer(out)) == 0
    return out


def test_the_restated_rank_rule_is_the_hosts_without_collisions():
    from doppel_speller_amd import _lib
    library = ctypes.CDLL(_lib.build_library())
    # twins of several sizes, rows with the same set and other sums32 bits, rows without columns (twins of each other)
    rng = np.random.RandomState(1)
    pool = [tuple(sorted(rng.choice(30, size=rng.randint(0, 6), replace=False).tolist())) for _ in range(40)]
    which = rng.randint(0, 40, 3000)
    sums32 = rng.choice(np.array([0.0, -0.0, 1.0, 2.5], dtype=np.float32), 3000)
    cols = [c for w in which for c in pool[w]]
    rows = [r for r, w in enumerate(which) for _ in pool[w]]
    rowptr, truth_idx = ic.csr_from_pairs(30, cols, rows)
    expected = _host_ranks(library, rowptr, truth_idx, sums32, 30, 3000)
    assert expected.max() > 5 and (expected == 0).sum() > 100
    assert np.array_equal(ic.duplicate_ranks_rule(rowptr, truth_idx, sums32), expected)
    # the internal order of an index: ranks are taken on it
    p_rowptr, p_idx, p_sums, original = ic.internal_csr(rowptr, truth_idx, sums32)
    assert np.array_equal(ic.duplicate_ranks_rule(p_rowptr, p_idx, p_sums), _host_ranks(library, p_rowptr, p_idx, p_sums, 30, 3000))
    assert np.array_equal(np.sort(original), np.arange(3000)) and np.all(np.diff(ic.order_key(p_sums).astype(np.int64)) >= 0)
    # the saturation of the twins problem of the GPU tests
    rowptr, truth_idx, _, sums32, v, n = ic.twins_problem()
    expected = _host_ranks(library, rowptr, truth_idx, sums32, v, n)
    assert expected.max() == 65535 and int((expected == 65535).sum()) == 70000 - 65535
    assert np.array_equal(ic.duplicate_ranks_rule(rowptr, truth_idx, sums32), expected)


def test_truncated_hashes_make_the_rule_differ_from_plain_twins():
    """With two hash bits distinct rows share groups: some real twins lose their rank (their group's largest row is another
    set) -- the restatement is not the collision-free answer there, which is what the GPU test relies on."""
    rowptr, truth_idx, _, sums32, v, n = ic.twins_problem()
    plain = ic.duplicate_ranks_rule(rowptr, truth_idx, sums32)
    cut = ic.duplicate_ranks_rule(rowptr, truth_idx, sums32, hash_bits=2)
    assert not np.array_equal(plain, cut) and np.all(cut <= plain)
    assert np.array_equal(ic.duplicate_ranks_rule(rowptr, truth_idx, sums32, hash_bits=64), plain)


def test_the_part_edges_problem_holds_what_it_claims():
    rowptr, truth_idx, idf32, sums32, v, n = ic.part_edges_problem("equal")
    assert (v, n) == (40, 2 * ic.NARROW + 100) and rowptr[26] == rowptr[25] and rowptr[27] - rowptr[26] == n
    for j in range(25):
        rows = truth_idx[rowptr[j]:rowptr[j + 1]].astype(np.int64)
        for tile in range(3):
            local = rows[rows // ic.NARROW == tile] % ic.NARROW
            assert (int((local % 2 == 0).sum()), int((local % 2 == 1).sum())) == ((0, 1, 3, 4, 5)[j % 5], (0, 1, 3, 4, 5)[j // 5])
    _, idx, _, runs, _, _ = ic.part_edges_problem("runs", full_column=False)
    assert np.setdiff1d(np.arange(n), idx).shape[0] > 1000                       # rows with no column at all
    ordered = np.sort(runs)
    assert ordered[ic.NARROW - 1] == ordered[ic.NARROW] and ordered[2 * ic.NARROW - 1] == ordered[2 * ic.NARROW]
    _, _, idf, signed, _, _ = ic.part_edges_problem("signed")
    bits = signed.view(np.uint32)
    assert (bits == 0x80000000).any() and (bits == 0).any() and (signed < 0).any() and (idf < 0).any()
