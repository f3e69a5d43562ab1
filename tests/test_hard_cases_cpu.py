"""Hard negatives without a GPU: the two restatements of the rule (tests/hard_cases.py) against each other, every named
case against the property it is named for, validate_hard's refusals, and the C ABI surface."""
import ctypes
import os

import numpy as np
import pytest

import hard_cases as hc
from doppel_speller_amd import _lib, training_set

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mined(case):
    return hc.mine_keys(*hc.arguments(case))


def _per_title(case):
    """{title: [positions in mined order]} of a case."""
    pair_q, _, position, _, _ = _mined(case)
    return {i: position[pair_q == case["q_first"] + i].tolist() for i in range(case["rows"].shape[0])}


@pytest.mark.parametrize("name", sorted(hc.CASES))
def test_the_two_restatements_agree(name):
    case = hc.CASES[name]
    by_sort, by_keys = hc.mine_sorted(*hc.arguments(case)), _mined(case)
    assert hc.same_mined(by_sort, by_keys)
    pair_q, pair_t, position, margin, total = by_keys
    assert total == pair_q.shape[0] <= case["rows"].shape[0] * case["hard_n"]
    assert (np.diff(pair_q) >= 0).all()                                 # dense, titles in order
    keys = hc.keys_of(*(case[n] for n in ("rows", "margins", "own", "exclude", "n_truth", "min_margin")))
    live = keys[keys != 0]
    assert all(np.unique(row[row != 0]).shape[0] == (row != 0).sum() for row in keys) and (live >> np.uint64(63)).size == live.size
    # cut into chunks, the titles' pairs are the same pairs
    n = case["rows"].shape[0]
    for size in (1, 2, 3):
        parts = [hc.mine_keys(*hc.arguments(hc.chunk_of(case, first, min(n, first + size)))) for first in range(0, n, size)]
        joined = tuple(np.concatenate([p[c] for p in parts]) for c in range(4)) + (sum(p[4] for p in parts),)
        assert hc.same_mined(joined, by_keys), size


def test_the_cases_cover_the_shapes_the_issue_names():
    cases = hc.CASES.values()
    assert {c["rows"].shape[1] for c in cases} >= {1, 5, 64, 65, 100, 130, 256, 257, 600}
    assert {c["hard_n"] for c in cases} >= {1, 3, 16}
    assert {c["rows"].shape[0] for c in cases} >= {1, 4, 5, 9}
    assert any(c["hard_n"] == c["rows"].shape[1] for c in cases)
    assert any(c["exclude"] is None for c in cases) and any(c["exclude"] is not None and c["exclude"].shape[1] == 0 for c in cases)
    assert hc.REGISTER_CANDIDATES == 256


def test_each_case_has_the_property_it_is_named_for():
    c = hc.CASES
    assert _mined(c["k1_single"])[2].tolist() == [0]

    case = c["k5_own_first"]
    assert (case["own"] == case["rows"][:, 0]).all() and all(0 not in p and len(p) == 3 for p in _per_title(case).values())
    assert _mined(case)[0].min() == 7                                   # q_first shows in pair_q
    case = c["k5_own_last"]
    assert (case["margins"][:, 4] > case["margins"][:, :4].max(axis=1)).all()      # the own row would have won
    assert all(sorted(p) == [0, 1, 2, 3] for p in _per_title(case).values())       # fewer eligible than hard_n = k

    case = c["k64_full"]
    assert case["own"].tolist()[1] not in case["rows"][1].tolist() and case["own"][0] == case["rows"][0, 63]
    assert [len(p) for p in _per_title(case).values()] == [16] * 5

    case = c["k65_ties"]
    assert (case["margins"][:, 63] == case["margins"][:, 64]).all() and (case["margins"][:, 64] == case["margins"].max(axis=1)).all()
    assert all(p == [10, 63, 64] for p in _per_title(case).values())               # the tie crosses lanes and the 64 edge
    assert all(p[:5] == [10, 63, 64, 1, 2] for p in _per_title(c["k65_ties_deep"]).values())

    case = c["k100_exclude"]
    free = _per_title(dict(case, exclude=None))
    held = _per_title(case)
    assert (case["exclude"][0] == -1).all() and held[0] == free[0]                 # -1 entries leave nothing out
    assert held[1] != free[1] and not set(case["exclude"][1, :2].tolist()) & set(case["rows"][1, held[1]].tolist())
    assert not set(case["exclude"][2].tolist()) & set(case["rows"][2].tolist()) and held[2] == free[2]
    assert held[3] != free[3] and (case["exclude"][3] == -1).sum() == 1
    assert all(case["own"][i] not in case["rows"][i, held[i]] for i in range(9))
    assert sum(case["own"][i] == case["rows"][i, np.argmax(case["margins"][i])] for i in range(9)) == 5

    case = c["k130_negative"]
    assert (case["margins"] < 0).all() and np.unique(case["margins"][0]).shape[0] < 130
    assert (np.diff(_mined(case)[3].reshape(5, 16), axis=1) <= 0).all()            # descending: -0.125 before -0.25
    assert any((np.diff(_mined(case)[3].reshape(5, 16), axis=1) == 0).any(axis=1))

    for k in (256, 257):
        assert all(p[0] == k - 1 for p in _per_title(c[f"k{k}_path_edge"]).values())

    case = c["k600_threshold"]
    lengths = [len(p) for p in _per_title(case).values()]
    assert lengths[1] == 2 and lengths[2] == 0 and lengths[0] > 0 and lengths[3] > 0    # short, empty between two with some
    assert _per_title(case)[1] == [5, 599]

    case = c["zeros"]
    assert np.signbit(case["margins"][0, 0]) and not np.signbit(case["margins"][0, 1])
    assert _per_title(case) == {0: [1, 3, 0], 1: [4, 0, 2]}                        # +0.0 before -0.0, each in order of j
    assert _per_title(c["zeros_threshold"]) == {0: [], 1: [4]}

    case = c["cut_at_the_threshold"]
    assert (case["margins"] == case["min_margin"]).sum() == 7
    assert _per_title(case) == {0: [3, 0], 1: []}                                  # equal to the threshold: left out

    case = c["invalid_rows"]
    assert {-1, -7, 30, 35} <= set(case["rows"][0].tolist()) and case["n_truth"] == 30
    assert all(not set(p) & {0, 5, 9, 16} and len(p) == 3 for p in _per_title(case).values())
    assert (case["margins"][:, [0, 5, 9, 16]] > np.delete(case["margins"], [0, 5, 9, 16], axis=1).max()).all()

    case = c["exclude_everything"]
    assert case["exclude"].shape[1] == 16 and case["hard_n"] == 16 == case["rows"].shape[1]
    assert [len(p) for p in _per_title(case).values()] == [16, 0, 2, 0, 16]

    assert _mined(c["nothing_mined"])[4] == 0 and (c["nothing_mined"]["margins"].max() == c["nothing_mined"]["min_margin"])
    assert _mined(c["nine_titles"])[4] == 9


def test_order_of_is_monotone_and_splits_the_zeros():
    values = np.array([-np.inf, -3.0, -1e-30, -0.0, 0.0, 1e-30, 2.5, np.inf], dtype=np.float32)
    order = hc.order_of(values).astype(np.int64)
    assert (np.diff(order) > 0).all()


# ---- validate_hard ------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the library was touched before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", refuse)


def stub_model(n_features=66, device=0, handle=True):
    """A ForestModel that never touched the library: what validate_hard looks at."""
    import doppel_speller_amd as ds

    class Stub(ds.ForestModel):
        def close(self):
            self.handle = None

    model = object.__new__(Stub)
    model.arrays, model.n_features, model.n_trees, model.device, model.cover = {}, n_features, 0, device, None
    model.handle = ctypes.c_void_p(1) if handle else None
    return model


def test_validate_hard(no_library):
    import doppel_speller_amd as ds
    assert ds.validate_hard is training_set.validate_hard and ds.DeviceHardNegatives is training_set.DeviceHardNegatives
    good = stub_model()
    assert ds.validate_hard(good, 5, None, True, 100, 10) == (5, float("-inf"))
    assert ds.validate_hard(good, np.int32(16), np.float32(0.5), False, 16, 10, device=0) == (16, 0.5)
    assert ds.validate_hard(good, 1, 2, np.bool_(True), 1, 1) == (1, 2.0)
    refusals = [
        (dict(model=None), "model must be a ForestModel"), (dict(model={"feature": []}), "model must be a ForestModel"),
        (dict(model=stub_model(handle=False)), "model is closed"), (dict(model=stub_model(n_features=7)), "model has 7 features"),
        (dict(model=stub_model(device=1), device=0), "model lives on device 1"),
        (dict(hard_n=0), "hard_n"), (dict(hard_n=17), "hard_n"), (dict(hard_n=True), "hard_n"), (dict(hard_n=2.0), "hard_n"),
        (dict(hard_n=None), "hard_n"), (dict(hard_n=11, top_n=10), "hard_n = 11 exceeds top_n = 10"),
        (dict(min_margin=float("nan")), "min_margin"), (dict(min_margin=float("inf")), "min_margin"),
        (dict(min_margin=float("-inf")), "min_margin"), (dict(min_margin="0.5"), "min_margin"),
        (dict(min_margin=True), "min_margin"),
        (dict(exclude_sampled=1), "exclude_sampled"), (dict(exclude_sampled=None), "exclude_sampled"),
        (dict(exclude_sampled="yes"), "exclude_sampled")]
    for change, message in refusals:
        arguments = dict(dict(model=good, hard_n=5, min_margin=None, exclude_sampled=True, top_n=100, sample_n=10), **change)
        with pytest.raises(ValueError, match=message):
            ds.validate_hard(**arguments)


def _engineering(**extra):
    import doppel_speller_amd as ds
    truth = ["alpha beta gamma", "delta epsilon", "zeta eta theta", "iota kappa"]
    return ds.FeatureEngineering(truth, [10, 11, 12, 13], ["alpha beta gama", "made up"], [10, -1], top_n=3, sample_n=2,
                                 **extra)


def test_a_missing_base_set_is_refused_before_the_library(no_library):
    fe = _engineering()
    for call in (fe.generate_hard_negatives, fe.generate_device_hard_negatives):
        with pytest.raises(ValueError, match="generate the base set .* first, or pass exclude_sampled=False"):
            call(stub_model(), hard_n=2)
        with pytest.raises(ValueError, match="hard_n = 4 exceeds top_n = 3"):
            call(stub_model(), hard_n=4, exclude_sampled=False)
        with pytest.raises(ValueError, match="model lives on device 1"):
            call(stub_model(device=1), hard_n=2)
    assert fe.hard_rows is None and fe.hard_timings == {} and fe.rows is None


def test_with_hard_negatives_checks_its_argument(no_library):
    import doppel_speller_amd as ds
    sets = ds.DeviceDataSets(None, 0, np.zeros(0, np.float32), None, 0, np.zeros(0, np.float32), None, None, 0)
    with pytest.raises(ValueError, match="must be a DeviceHardNegatives"):
        sets.with_hard_negatives((np.zeros((0, 66), np.float32), np.zeros(0, np.float32)))


# ---- the C ABI ----------------------------------------------------------------------------------------------------------
def test_header_and_sources_declare_the_entry_points():
    with open(os.path.join(ROOT, "include", "doppel_amd.h")) as handle:
        header = " ".join(handle.read().split())
    assert ("int ds_hard_negatives_device(const int32_t *d_rows, const float *d_margins, int64_t n_queries, int32_t k, "
            "int64_t n_truth, const int32_t *d_own_row, const int32_t *d_exclude, int32_t n_exclude, int32_t hard_n, "
            "float min_margin, int64_t q_first, int64_t *d_offsets, int64_t *d_total, int64_t capacity, "
            "int32_t *d_pair_q, int32_t *d_pair_t, int32_t *d_position, float *d_margin, void *stream);") in header
    assert "int ds_hard_option(const char *name, int64_t value);" in header
    assert "int ds_hard_total(const int64_t *d_total, int64_t *total, void *stream);" in header
    assert {"ds_hard_negatives_device", "ds_hard_option", "ds_hard_total"} <= set(_lib.EXPORTED_SYMBOLS)
    assert "ds_hard.hip" in _lib._SOURCES


def test_the_entry_refuses_bad_arguments_without_a_device():
    import doppel_speller_amd as ds
    library = ctypes.CDLL(ds.build_library())
    library.ds_last_error.restype = ctypes.c_char_p
    c = ctypes
    library.ds_hard_negatives_device.argtypes = [c.c_void_p, c.c_void_p, c.c_int64, c.c_int32, c.c_int64, c.c_void_p,
                                                 c.c_void_p, c.c_int32, c.c_int32, c.c_float, c.c_int64, c.c_void_p,
                                                 c.c_void_p, c.c_int64] + [c.c_void_p] * 5
    library.ds_hard_option.argtypes = [c.c_char_p, c.c_int64]
    somewhere = c.c_void_p(0x1000)          # never read: every call below is refused before any device work

    def call(n_queries=4, k=100, n_truth=50, exclude=None, n_exclude=0, hard_n=5, min_margin=0.0, q_first=0, capacity=20,
             pointers=(somewhere,) * 9):
        rows, margins, own, offsets, total, pair_q, pair_t, position, margin = pointers
        return library.ds_hard_negatives_device(rows, margins, n_queries, k, n_truth, own, exclude, n_exclude, hard_n,
                                                min_margin, q_first, offsets, total, capacity, pair_q, pair_t, position,
                                                margin, None)

    for at in range(9):
        assert call(pointers=tuple(None if i == at else somewhere for i in range(9))) == -1, at
        assert b"ds_hard_negatives_device: null pointer" in library.ds_last_error()
    for hard_n, k in ((0, 100), (-1, 100), (17, 100), (6, 5), (2, 1)):
        assert call(hard_n=hard_n, k=k) == -1
        assert b"hard_n = %d out of range" % hard_n in library.ds_last_error()
    assert call(k=0, hard_n=1) == -1 and b"k = 0" in library.ds_last_error()
    for n_exclude in (-1, 17):
        assert call(n_exclude=n_exclude, exclude=somewhere) == -1
        assert b"n_exclude = %d out of range" % n_exclude in library.ds_last_error()
    assert call(n_exclude=3, exclude=None) == -1 and b"n_exclude = 3 with a null d_exclude" in library.ds_last_error()
    for change in (dict(n_queries=-1), dict(n_truth=-1), dict(q_first=-1), dict(capacity=-1)):
        assert call(**change) == -1 and b"negative count" in library.ds_last_error()
    assert call(min_margin=float("nan")) == -1 and b"NaN" in library.ds_last_error()
    assert call(q_first=2 ** 31 - 2) == -1 and b"int32" in library.ds_last_error()
    assert call(n_queries=0) == 0                                       # nothing to do: DS_OK, nothing launched
    assert library.ds_hard_total(None, None, None) == -1 and b"ds_hard_total: null pointer" in library.ds_last_error()
    assert library.ds_hard_option(None, 1) == -1 and library.ds_hard_option(b"no_such_option", 1) == -1
    assert library.ds_hard_option(b"max_blocks", -1) == -1 and library.ds_hard_option(b"max_blocks", 65537) == -1
    assert library.ds_hard_option(b"max_blocks", 1) == 0 and library.ds_hard_option(b"max_blocks", 0) == 0
