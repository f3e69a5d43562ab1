"""The paired bootstrap without a GPU ("Is a difference real: the paired bootstrap"): the oracle's
draws against big-integer arithmetic, properties of the rule, the statistics, every refusal of validate_bootstrap, the
classification of bootstrap_accuracy, what the shared cases cover, the C ABI surface and the library's refusals."""
import ctypes
import os
import re

import numpy as np
import pytest

import bootstrap_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the draws -----------------------------------------------------------------------------------------------------------
def _seed_with_top_bit(b, k):
    """A seed whose x(b, k) has its top bit set (found by search, so that the pick is made from the rule itself)."""
    for seed in range(1000):
        if oracle.stream_first(seed, 7, (b << 32) | k) >> 63:
            return seed
    raise AssertionError("no seed found")


def test_index_against_big_integers():
    from training_set_oracle import Stream
    picks = [(0, 0, 0, 1), (5, 3, 0, 1), (1, 0, 0, 2), (1, 7, 1, 2), (12345, 65535, 999, 1000), ((1 << 63) - 1, 65535, 12, 13),
             (99, 1, (1 << 31) - 1, 1 << 31), (99, 65535, 0, 1 << 31), (7, 2, 40, 11141),
             (_seed_with_top_bit(3, 5), 3, 5, 1 << 31), (_seed_with_top_bit(0, 0), 0, 0, 3)]
    assert oracle.stream_first(picks[-2][0], 7, (3 << 32) | 5) >> 63 == 1
    for seed, b, k, n_units in picks:
        x = Stream(seed, 7, (b << 32) | k).next()                   # the project's stream, in Python integers
        assert oracle.stream_first(seed, 7, (b << 32) | k) == x
        expected = (x * n_units) >> 64
        assert 0 <= expected < n_units and oracle.draw_one(seed, b, k, n_units) == expected
        index = np.array([(b << 32) | k], np.uint64)
        assert int(oracle.stream_first_array(seed, 7, index)[0]) == x
        assert int(oracle.high_product(np.array([x], np.uint64), n_units)[0]) == expected
    for seed, b, n_units in ((3, 0, 1), (3, 9, 2), (8, 65535, 257), ((1 << 63) - 1, 4, 1000)):
        assert oracle.draws(seed, b, n_units).tolist() == [oracle.draw_one(seed, b, k, n_units) for k in range(n_units)]
    x = np.array([0, 1, (1 << 64) - 1, 1 << 63, (1 << 63) - 1, 0xffffffff, 1 << 32], np.uint64)
    for n_units in (1, 2, 3, (1 << 31) - 1, 1 << 31):
        assert oracle.high_product(x, n_units).tolist() == [(int(v) * n_units) >> 64 for v in x]


def test_draws_differ_between_replicates_and_seeds():
    base = oracle.draws(7, 0, 1000)
    assert np.array_equal(base, oracle.draws(7, 0, 1000))
    for other in (oracle.draws(7, 1, 1000), oracle.draws(8, 0, 1000)):
        assert np.count_nonzero(other != base) > 900
    assert abs(np.bincount(oracle.draws(1, 2, 100000) // 10000, minlength=10) - 10000).max() < 500   # about uniform


# ---- properties of the rule ------------------------------------------------------------------------------------------------------
def test_one_unit_makes_every_replicate_the_baseline():
    c = oracle.case("units_1")
    assert c["n_units"] == 1 and (c["counts"] == c["baseline"][None]).all() and c["baseline"].sum() == c["n"] * c["n_sets"]


@pytest.mark.parametrize("name", oracle.NAMES)
def test_counts_sum_to_the_sizes_of_the_drawn_units(name):
    c = oracle.case(name)
    sizes = oracle.unit_sizes(c)
    assert c["counts"].shape == (c["n_boot"], c["n_sets"], 4) and c["counts"].dtype == np.int64
    assert (c["baseline"].sum(axis=1) == c["n"]).all()
    for b in range(c["n_boot"]):
        drawn = int(sizes[oracle.draws(c["seed"], b, c["n_units"])].sum())
        assert (c["counts"][b].sum(axis=1) == drawn).all()
        if c["unit"] is None:
            assert drawn == c["n"]


def test_identical_sets_have_identical_counts():
    rng = np.random.RandomState(5)
    codes = rng.randint(0, 4, (3, 500)).astype(np.uint8)
    codes[2] = codes[0]
    unit = rng.randint(0, 40, 500).astype(np.int32)
    for u, n_units in ((None, 500), (unit, 40)):
        got, baseline = oracle.counts(codes, u, n_units, 20, 9)
        assert np.array_equal(got[:, 0], got[:, 2]) and not np.array_equal(got[:, 0], got[:, 1])
        assert np.array_equal(baseline[0], baseline[2])
    one, _ = oracle.counts(codes[:1], unit, 40, 20, 9)
    assert np.array_equal(one[:, 0], got[:, 0])                       # a set's counts do not depend on the other sets


def test_prefix_of_the_replicates():
    c = oracle.case("units_65")
    fewer, _ = oracle.counts(c["codes"], c["unit"], c["n_units"], 4, c["seed"])
    assert np.array_equal(fewer, c["counts"][:4])


# ---- the statistics ------------------------------------------------------------------------------------------------------------
def test_statistics_on_crafted_arrays():
    import doppel_speller_amd as ds
    counts = np.zeros((4, 3, 4), np.int64)
    counts[:, 0, 2] = [10, 12, 14, 16]                                 # errors 10, 12, 14, 16
    counts[:, 1, 2] = [10, 12, 14, 16]                                 # tied with set 0 in every replicate
    counts[:, 2, 1] = [1, 2, 3, 5]                                     # errors 5, 10, 15, 25 at weight 5
    baseline = counts[0].copy()
    got = ds.ErrorBootstrap(counts, baseline, 5.0, names=("a", "b", "c"), n_units=7, seed=3)
    assert got.errors.tolist() == [[10, 10, 5], [12, 12, 10], [14, 14, 15], [16, 16, 25]]
    assert got.baseline_errors.tolist() == [10, 10, 5] and got.n_boot == 4 and got.n_units == 7
    assert np.array_equal(got.errors, oracle.errors(counts, 5.0))
    assert got.interval(0.5).tolist() == [[11.5, 14.5], [11.5, 14.5], [8.75, 17.5]]
    assert got.interval().tobytes() == np.stack([oracle.interval(got.errors[:, m], 0.95) for m in range(3)]).tobytes()
    assert got.standard_error.tolist() == [oracle.standard_error(got.errors[:, m]) for m in range(3)]
    assert got.standard_error[0] == np.std([10, 12, 14, 16], ddof=1)
    ties = got.difference("a", "b")
    assert ties.share_better == 0.5 and ties.mean == 0 and ties.interval == (0.0, 0.0) and ties.baseline == 0
    d = got.difference(0, "c", level=0.5)
    expected = oracle.difference(got.errors, 0, 2, 0.5)
    assert d.differences.tolist() == [5, 2, -1, -9] and d.share_better == 0.5 and d.mean == expected["mean"] == -0.75
    assert d.interval == expected["interval"] and d.standard_error == expected["standard_error"] and d.baseline == 5
    assert got.difference("c", "a").share_better == 0.5 and got.difference(0, 2).differences.tolist() == [5, 2, -1, -9]
    counts[3, 2, 1] = 3                                                # 16 against 15: a is worse in one more
    assert ds.ErrorBootstrap(counts, baseline, 5.0).difference(0, 2).share_better == 0.25
    with pytest.raises(ValueError, match="not one of the names"):
        got.difference("a", "z")
    with pytest.raises(ValueError, match="set must be"):
        got.difference(0, 3)
    frame = got.frame()
    assert frame["name"].tolist() == ["a", "b", "c"] and frame["baseline_error"].tolist() == [10, 10, 5]
    assert frame["fn"].tolist() == [10, 10, 0] and frame["fp"].tolist() == [0, 0, 1]
    assert frame["low"].tolist() == got.interval()[:, 0].tolist()


def test_one_replicate_has_standard_error_zero():
    import doppel_speller_amd as ds
    counts = np.arange(8, dtype=np.int64).reshape(1, 2, 4)
    got = ds.ErrorBootstrap(counts, counts[0], 5.0)
    assert got.standard_error.tolist() == [0.0, 0.0] and oracle.standard_error(got.errors[:, 0]) == 0.0
    assert got.difference(0, 1).standard_error == 0.0 and got.names == ("set0", "set1")
    assert got.interval().tolist() == [[7.0, 7.0], [31.0, 31.0]]


# ---- validate_bootstrap ----------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    from doppel_speller_amd import _lib

    def refuse():
        raise AssertionError("the library was called before the arguments were validated")
    monkeypatch.setattr(_lib, "lib", refuse)


def _model(n_features=7, device=0, handle=1):
    import doppel_speller_amd as ds
    model = ds.ForestModel.__new__(ds.ForestModel)
    model.n_features, model.device, model.handle = n_features, device, handle
    return model


CODES = np.array([[0, 1, 2, 3], [3, 3, 0, 0]])


@pytest.mark.parametrize("arguments, message", [
    (dict(codes=np.zeros((2, 2, 2), np.int64)), "codes must be an"),
    (dict(codes=np.zeros((2, 4))), "codes must be integers"),
    (dict(codes=np.zeros((2, 4), bool)), "codes must be integers"),
    (dict(codes=[[0, 1, 4, 3]]), r"codes\[0\]\[2\] = 4"),
    (dict(codes=[[0, 1, 2, 3], [0, -1, 2, 3]]), r"codes\[1\]\[1\] = -1"),
    (dict(codes=np.zeros((0, 4), np.int64)), "0 prediction sets"),
    (dict(codes=np.zeros((65, 4), np.int64)), "65 prediction sets"),
    (dict(n=5), "n = 5 but codes has 4"),
    (dict(n_boot=0), "n_boot"),
    (dict(n_boot=65537), "n_boot"),
    (dict(n_boot=2.0), "n_boot"),
    (dict(n_boot=True), "n_boot"),
    (dict(seed=-1), "seed"),
    (dict(seed=1 << 63), "seed"),
    (dict(groups=[1, 2, 3]), "groups must hold 4"),
    (dict(groups=[1, 2, 3, 4, 5]), "groups must hold 4"),
    (dict(groups=np.zeros((4, 1), np.int64)), "groups must hold 4"),
    (dict(groups=[1.0, 2.0, 3.0, 4.0]), "groups must be integers or strings"),
    (dict(groups=[True, False, True, False]), "groups must be integers or strings"),
    (dict(groups=np.array(["a", "b", 3, "c"], dtype=object)), "an object array: of strings only"),
    (dict(groups=np.array([1, 2, 3, 4], dtype=object)), "an object array: of strings only"),
    (dict(level=0), "level"),
    (dict(level=1), "level"),
    (dict(level=float("nan")), "level"),
    (dict(level="high"), "level"),
    (dict(threshold=0), "threshold"),
    (dict(threshold=1.0), "threshold"),
    (dict(beta=0), "beta"),
    (dict(beta=float("inf")), "beta"),
    (dict(names=("a",)), "1 names for 2"),
    (dict(names=("a", "a")), "distinct strings"),
    (dict(names="ab"), "names must be a sequence"),
    (dict(names=(1, 2)), "distinct strings"),
])
def test_validate_bootstrap_refuses(no_library, arguments, message):
    import doppel_speller_amd as ds
    with pytest.raises(ValueError, match=message):
        ds.validate_bootstrap(**dict(dict(codes=CODES), **arguments))


def test_validate_bootstrap_refuses_models(no_library):
    import doppel_speller_amd as ds
    for models, message in (([], "0 models"), ([_model()] * 65, "65 models"), (_model(), "models must be a list"),
                            ([_model(), "model"], r"models\[1\] must be a ForestModel"),
                            ([_model(), _model(handle=None)], r"models\[1\] is closed"),
                            ([_model(), _model(n_features=8)], r"models\[1\] has 8 features, not 7"),
                            ([_model(), _model(device=1)], r"models\[1\] lives on device 1")):
        with pytest.raises(ValueError, match=message):
            ds.validate_bootstrap(models=models, n=4)
    with pytest.raises(ValueError, match=r"models\[0\] has 7 features, not 66"):
        ds.validate_bootstrap(models=[_model()], n=4, n_features=66)
    with pytest.raises(ValueError, match="n must be"):
        ds.validate_bootstrap(models=[_model()], n=(1 << 31) + 1)
    with pytest.raises(ValueError, match="n must be"):
        ds.validate_bootstrap(models=[_model()], n=-1)
    rows = np.zeros((4, 7), np.float32)
    for call, message in ((lambda: ds.compare_models([_model()], np.zeros((4, 6)), [0, 1, 0, 1]), "rows must be a"),
                          (lambda: ds.compare_models([_model()], np.zeros(7), [0]), "rows must be a"),
                          (lambda: ds.compare_models([_model()], rows, [0, 1, 0]), "target must hold 4"),
                          (lambda: ds.compare_models([_model()], rows, [0, 1, 2, 0]), "target labels"),
                          (lambda: ds.compare_models([_model()], rows, [0, 1, 0, 1], groups=[1, 2]), "groups must hold 4"),
                          (lambda: ds.compare_models([], rows, [0, 1, 0, 1]), "0 models"),
                          (lambda: ds.compare_models(None, rows, [0, 1, 0, 1]), "models are missing"),
                          (lambda: ds.compare_models_device([_model()], None, 4, None), "device matrix"),
                          (lambda: ds.compare_models_device([_model()], None, 4, None, n_boot=0), "n_boot"),
                          (lambda: ds.bootstrap_counts(None), "codes are missing"),
                          (lambda: ds.bootstrap_counts(CODES, n_boot=0), "n_boot"),
                          (lambda: ds.bootstrap_accuracy({}, [1, 2]), "0 prediction sets"),
                          (lambda: ds.bootstrap_accuracy(np.zeros(3), [1, 2, 3]), "dict or a list"),
                          (lambda: ds.bootstrap_accuracy([[1, 2, 3]], [1, 2]), "3 predicted ids but 2"),
                          (lambda: ds.bootstrap_accuracy([[1, 2]], [1, 2], groups=[1]), "groups must hold 2")):
        with pytest.raises(ValueError, match=message):
            call()


def test_validate_bootstrap_accepts(no_library):
    import doppel_speller_amd as ds
    v = ds.validate_bootstrap(codes=CODES, groups=["b", "a", "b", "c"], n_boot=65536, seed=(1 << 63) - 1, level=0.5,
                              names=("x", "y"))
    assert v["codes"].dtype == np.uint8 and v["codes"].flags["C_CONTIGUOUS"] and (v["n"], v["n_sets"]) == (4, 2)
    assert v["unit"].dtype == np.int32 and v["unit"].tolist() == [0, 1, 0, 2] and v["n_units"] == 3
    import pandas as pd
    v = ds.validate_bootstrap(codes=CODES, groups=pd.Series(["b", "a", "b", "c"]).to_numpy())   # an object array
    assert v["unit"].tolist() == [0, 1, 0, 2] and v["n_units"] == 3
    v = ds.validate_bootstrap(codes=[0, 3, 3], groups=np.array([7, 7, -2]), n_boot=1)
    assert v["codes"].shape == (1, 3) and v["unit"].tolist() == [0, 0, 1] and v["n_units"] == 2
    v = ds.validate_bootstrap(models=[_model(), _model()], n=1 << 31)
    assert v["n_units"] == 1 << 31 and v["unit"] is None and v["n_sets"] == 2 and v["n_features"] == 7
    v = ds.validate_bootstrap(codes=np.zeros((1, 0), np.int64))
    assert v["n"] == 0 and v["n_units"] == 0
    rng = np.random.RandomState(1)
    groups = rng.randint(-50, 50, 400)
    from doppel_speller_amd.bootstrap import dense_units
    unit, n_units = dense_units(groups)
    expected, expected_units = oracle.dense_units(groups)
    assert unit.tolist() == expected.tolist() and n_units == expected_units
    unit, n_units = dense_units(np.array(["t%d" % g for g in groups]))
    assert unit.tolist() == expected.tolist()


@pytest.mark.parametrize("change, message", [
    (dict(bootstrap_repeats=-1), r"bootstrap_repeats must be an integer in \[0, 65536\]"),
    (dict(bootstrap_repeats=2.0), r"bootstrap_repeats must be an integer in \[0, 65536\]"),
    (dict(bootstrap_repeats=True), r"bootstrap_repeats must be an integer in \[0, 65536\]"),
    (dict(bootstrap_repeats=(1 << 16) + 1), r"bootstrap_repeats must be an integer in \[0, 65536\]"),
    (dict(bootstrap_repeats=2, bootstrap_seed=-1), r"bootstrap_seed must be an integer in \[0, "),
    (dict(bootstrap_repeats=2, bootstrap_seed=1 << 63), r"bootstrap_seed must be an integer in \[0, "),
    (dict(bootstrap_repeats=2, evaluation_fractions=dict(generated=0, negative=0, positive=0)),
     "bootstrap_repeats needs an evaluation set"),
])
def test_train_model_validates_bootstrap_arguments(no_library, change, message):
    import doppel_speller_amd as ds
    good = dict(truth_titles=["alpha beta", "gamma delta", "epsilon zeta"], truth_title_ids=[5, 6, 7],
                train_titles=["alpha bet", "unknown"], train_title_ids=[5, -1], top_n=2, sample_n=1)
    with pytest.raises(ValueError, match=message):
        ds.train_model(**dict(good, **change))


# ---- bootstrap_accuracy's classification ------------------------------------------------------------------------------------------
def test_accuracy_codes_follow_predictions_accuracy():
    import doppel_speller_amd as ds
    from doppel_speller_amd.bootstrap import ACCURACY_CODES, accuracy_codes
    predicted = np.array([5, 6, -1, -1, 9, -1, 7])
    actual = np.array([5, 7, -1, 8, 9, -1, -1])
    codes = accuracy_codes(predicted, actual)
    assert codes.tolist() == [3, 1, 0, 2, 3, 0, 1] == oracle.accuracy_codes(predicted, actual).tolist()
    report = ds.predictions_accuracy(predicted, actual)
    counts = np.bincount(codes, minlength=4)
    assert {name: int(counts[c]) for c, name in enumerate(ACCURACY_CODES)} == {k: report[k] for k in ACCURACY_CODES}
    assert counts[2] + 5 * counts[1] == report["custom_error"]
    for p, a, code in ((3, 3, 3), (3, 4, 1), (3, -1, 1), (-1, -1, 0), (-1, 4, 2)):       # the four outcomes one by one
        assert accuracy_codes([p], [a]).tolist() == [code]
        assert ds.predictions_accuracy([p], [a])[ACCURACY_CODES[code]] == 1


# ---- what the cases cover -------------------------------------------------------------------------------------------------------------
def test_cases_cover_the_shapes():
    built = {name: oracle.case(name) for name in oracle.NAMES}
    grouped = {name: c for name, c in built.items() if c["unit"] is not None}
    rows = {name: c for name, c in built.items() if c["unit"] is None}
    for side in (grouped, rows):
        assert {1, 2, 63, 64, 65, 255, 256, 257} <= {c["n_units"] for c in side.values()}
        assert {1, 2, 5, 64} <= {c["n_sets"] for c in side.values()}
        assert any(c["n_boot"] == 1 for c in side.values())
        assert any(c["n_boot"] % oracle.REPLICATES_PER_BLOCK == 1 and c["n_boot"] > 1 for c in side.values())
    assert all(c["n_units"] == c["n"] for c in rows.values())
    big = [c for c in built.values() if c["n_sets"] == 64]
    assert all(c["n_units"] == 65 and c["n_boot"] == 3 for c in big)
    empty = {name for name, c in grouped.items() if (oracle.unit_sizes(c) == 0).any()}
    assert {"units_63", "units_64", "units_255", "units_256", "units_one_holds_all", "units_hbm"} <= empty
    assert "units_1" not in empty and "units_overflow" not in empty
    unequal = {name for name, c in grouped.items() if np.unique(oracle.unit_sizes(c)).shape[0] > 2}
    assert {"units_63", "units_65", "units_257", "units_hbm"} <= unequal
    holds_all = {name for name, c in grouped.items() if oracle.unit_sizes(c).max() == c["n"]}
    assert holds_all == {"units_1", "units_one_holds_all"} and built["units_one_holds_all"]["n_units"] == 7
    beyond_lds = {name for name, c in built.items() if oracle.table_bytes(c) > oracle.LDS_TABLE_BYTES}
    assert beyond_lds == {"rows_hbm", "rows_chunks", "units_hbm"}
    assert 16384 < built["rows_two_chunks"]["n"] and oracle.table_bytes(built["rows_two_chunks"]) == 80000
    assert all(oracle.table_bytes(built[name]) <= 4 << 20 and built[name]["n_boot"] <= 3 for name in beyond_lds)
    # the overflow cases: one class of one set gets more than 2^16 in a replicate
    over = built["units_overflow"]
    assert sorted(oracle.unit_sizes(over).tolist()) == [1, 70001] and (over["codes"] == 1).all()
    assert over["counts"][:, 0, 1].max() == 2 * 70001 and over["counts"][:, 0, 1].min() <= 70002
    assert (built["rows_chunks"]["counts"][:, 0, 1] == 70001).all() and 70001 > 1 << 16


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_header_and_symbol_lists():
    from doppel_speller_amd import _lib, bootstrap
    header = open(os.path.join(ROOT, "include", "doppel_amd.h")).read()
    assert re.search(r"int ds_bootstrap_counts_device\(const uint8_t \*d_codes, int32_t n_sets, int64_t n, "
                     r"const int32_t \*d_unit, int64_t n_units,\s+int32_t n_boot, uint64_t seed, long long \*d_counts, "
                     r"long long \*d_baseline, void \*stream\);", header)
    assert re.search(r"int ds_bootstrap_counts\(const uint8_t \*codes, int32_t n_sets, int64_t n, const int32_t \*unit, "
                     r"int64_t n_units,\s+int32_t n_boot, uint64_t seed, long long \*counts, long long \*baseline\);", header)
    assert re.search(r"int ds_bootstrap_option\(const char \*name, int64_t value\);", header)
    assert re.search(r"int ds_outcome_codes_device\(const float \*d_margins, const float \*d_target, int64_t n, "
                     r"double threshold, uint8_t \*d_codes,\s+void \*stream\);", header)
    assert re.search(r"#define DS_BOOTSTRAP_PURPOSE_DRAW 7\b", header)
    purposes = re.findall(r"#define DS_[A-Z_]*PURPOSE[A-Z_]* (\d+)", header)
    assert len(purposes) == len(set(purposes)) and "7" in purposes
    assert bootstrap.PURPOSE_DRAW == oracle.PURPOSE_DRAW == 7
    assert (bootstrap.SETS_MAX, bootstrap.BOOT_MAX, bootstrap.ROWS_MAX) == (oracle.SETS_MAX, oracle.BOOT_MAX, oracle.ROWS_MAX)
    assert {"ds_bootstrap_counts_device", "ds_bootstrap_counts", "ds_bootstrap_option",
            "ds_outcome_codes_device"} <= set(_lib.EXPORTED_SYMBOLS)
    assert len(set(_lib.EXPORTED_SYMBOLS)) == len(_lib.EXPORTED_SYMBOLS)
    assert "ds_bootstrap.hip" in _lib._SOURCES and len(set(_lib._SOURCES)) == len(_lib._SOURCES)


@pytest.fixture(scope="module")
def library():
    import doppel_speller_amd as ds
    from doppel_speller_amd import _lib
    handle = _lib._declare(ctypes.CDLL(ds.build_library()))
    return handle


def _p(array):
    return None if array is None else array.ctypes.data_as(ctypes.c_void_p)


def test_library_refuses_without_gpu(library):
    """Everything the library can refuse before it touches a device: limits one past each bound, null pointers, and
    in the host form a bad code or unit; the outputs stay as they were."""
    codes = np.array([[0, 1, 2, 3], [3, 3, 0, 0]], np.uint8)
    unit = np.array([0, 1, 1, 2], np.int32)
    counts = np.full((3, 2, 4), 77, np.int64)
    baseline = np.full((2, 4), 77, np.int64)

    def host(codes_=codes, n_sets=2, n=4, unit_=unit, n_units=3, n_boot=3, counts_=counts, baseline_=baseline):
        return library.ds_bootstrap_counts(_p(codes_), n_sets, n, _p(unit_), n_units, n_boot, 5, _p(counts_), _p(baseline_))

    def device(codes_=codes, n_sets=2, n=4, unit_=unit, n_units=3, n_boot=3, counts_=counts, baseline_=baseline):
        return library.ds_bootstrap_counts_device(_p(codes_), n_sets, n, _p(unit_), n_units, n_boot, 5, _p(counts_),
                                                  _p(baseline_), None)

    for call, name in ((host, b"ds_bootstrap_counts:"), (device, b"ds_bootstrap_counts_device:")):
        for arguments, message in ((dict(n_sets=0), b"n_sets = 0"), (dict(n_sets=65), b"n_sets = 65"),
                                   (dict(n_boot=0), b"n_boot = 0"), (dict(n_boot=65537), b"n_boot = 65537"),
                                   (dict(n=-1), b"n = -1"), (dict(n=(1 << 31) + 1), b"outside [0, 2^31]"),
                                   (dict(n_units=0), b"n_units = 0"), (dict(n_units=(1 << 31) + 1), b"n_units = 2147483649"),
                                   (dict(unit_=None), b"every one of the 4 rows is its own unit"),
                                   (dict(unit_=None, n_units=5), b"n_units = 5"),
                                   (dict(codes_=None), b"null pointer"), (dict(counts_=None), b"null pointer"),
                                   (dict(baseline_=None), b"null pointer")):
            assert call(**arguments) == -1, arguments
            error = library.ds_last_error()
            assert error.startswith(name) and message in error, (arguments, error)
    bad = codes.copy()
    bad[1, 2] = 4
    assert host(codes_=bad) == -1 and b"code 4 of row 2 of set 1" in library.ds_last_error()
    for value in (-1, 3):
        units = unit.copy()
        units[3] = value
        assert host(unit_=units) == -1 and b"unit[3] = %d is outside [0, 3)" % value in library.ds_last_error()
    assert (counts == 77).all() and (baseline == 77).all()
    assert host(codes_=None, n=0) == 0 and not counts.any() and not baseline.any()   # no rows: zeroed, no device needed
    margins, target, out = np.zeros(4, np.float32), np.zeros(4, np.float32), np.full(4, 9, np.uint8)

    def outcome(margins_=margins, target_=target, n=4, threshold=0.9, out_=out):
        return library.ds_outcome_codes_device(_p(margins_), _p(target_), n, threshold, _p(out_), None)
    for arguments, message in ((dict(n=-1), b"n = -1"), (dict(n=(1 << 31) + 1), b"outside [0, 2^31]"),
                               (dict(threshold=0.0), b"threshold"), (dict(threshold=1.0), b"threshold"),
                               (dict(threshold=float("nan")), b"threshold"), (dict(margins_=None), b"null pointer"),
                               (dict(target_=None), b"null pointer"), (dict(out_=None), b"null pointer")):
        assert outcome(**arguments) == -1, arguments
        assert library.ds_last_error().startswith(b"ds_outcome_codes_device:") and message in library.ds_last_error()
    assert outcome(n=0) == 0 and (out == 9).all()
    for name, value in ((b"max_blocks", -1), (b"max_blocks", 65536), (b"replicates_per_block", -1),
                        (b"replicates_per_block", 65538), (b"table_in_lds", 2), (b"no_such", 0), (None, 0)):
        assert library.ds_bootstrap_option(name, value) == -1 and b"ds_bootstrap_option" in library.ds_last_error()
    for name, value in ((b"max_blocks", 3), (b"max_blocks", 0), (b"replicates_per_block", 7), (b"replicates_per_block", 0),
                        (b"table_in_lds", 0), (b"table_in_lds", 1)):
        assert library.ds_bootstrap_option(name, value) == 0
