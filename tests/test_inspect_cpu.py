"""Model inspection without a GPU ("Model inspection"): the closed-form permutation, the oracle's
forest walk, the conditions the cases must meet, validate_inspection, the C ABI surface and the library's refusals."""
import ctypes
import os
import re

import numpy as np
import pytest

import forest_inspect_oracle as oracle
import inspect_cases as cases
from test_forest_cpu import _python_predict, random_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the permutation ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 16, 17, 255, 256, 257, 1000, 65537])
def test_perm_is_a_bijection(n):
    for feature, repeat in ((0, 0), (65, 3), (95, 65535)):
        image = oracle.perm(12345, feature, repeat, n)
        assert image.shape == (n,) and np.array_equal(np.sort(image), np.arange(n))


def test_perm_differs_between_features_repeats_and_seeds():
    base = oracle.perm(7, 3, 0, 1000)
    for other in (oracle.perm(7, 4, 0, 1000), oracle.perm(7, 3, 1, 1000), oracle.perm(8, 3, 0, 1000)):
        assert np.count_nonzero(other != base) > 900
    assert np.array_equal(base, oracle.perm(7, 3, 0, 1000))


def test_perm_shuffles():
    image = oracle.perm(1, 0, 0, 65537)
    assert np.count_nonzero(image == np.arange(65537)) < 10            # a random permutation has one on average


def test_perm_array_form_equals_the_scalar_rule():
    for n in (2, 5, 17, 300):
        image = oracle.perm(99, 65, 2, n)
        assert [oracle.perm_one(99, 65, 2, n, i) for i in range(n)] == image.tolist()
    assert oracle.perm_one(5, 1, 1, 1, 0) == 0
    assert [oracle.half_bits(n) for n in (2, 3, 4, 5, 16, 17, 256, 257, 1 << 31)] == [1, 1, 1, 2, 2, 3, 4, 5, 16]


def test_round_keys_come_from_the_projects_stream():
    from training_set_oracle import Stream
    for seed, feature, repeat in ((0, 0, 0), (12345, 65, 3), ((1 << 63) - 1, 95, 65535)):
        for j, key in enumerate(oracle.round_keys(seed, feature, repeat)):
            index = (repeat << 40) | (feature << 32) | j
            assert key == Stream(seed, 6, index).next()
    assert oracle.mix64(0) == 0 and oracle.mix64(0x9e3779b97f4a7c15) == 0xe220a8397b1dcdaf   # splitmix64(0)'s first output


# ---- the oracle's walk and the cases -----------------------------------------------------------------------------------------
def test_vectorised_walk_equals_the_python_walk():
    forest = cases.forest_of(5, 12, 66, 6)
    rows = random_rows(6, 120)
    expected = np.array([_python_predict(forest, row) for row in rows], dtype=np.float32)
    assert oracle.margins(forest, rows).tobytes() == expected.tobytes()


def test_counters_of_known_margins():
    margin = np.array([10.0, -10.0, np.nan, 3000.0, -3000.0, 0.5], np.float32)
    target = np.array([1, 1, 1, 0, 0, 0], np.float32)
    got = oracle.counters_of(margin, target, 0.9)
    assert got[:4] == [1, 2, 1, 2]                                     # the NaN row is a missed positive
    assert got[4] == (10 << 20) - (10 << 20) + (2048 << 20) - (2048 << 20) + (1 << 19)
    assert oracle.counters_of(margin, None, 0.9)[:4] == [0, 4, 2, 0]


@pytest.mark.parametrize("name", cases.NAMES)
def test_case_conditions(name):
    case = cases.case(name)
    n = case["rows"].shape[0]
    assert case["gap"] >= cases.PROBABILITY_GAP, (name, case["gap"])
    assert case["expected"].shape == (len(case["jobs"]), 5) and case["expected"].dtype == np.uint64
    assert (case["expected"][:, :4].sum(axis=1) == n).all()
    if case["target"] is None or not case["target"].any():
        assert not case["expected"][:, [0, 3]].any()
    elif case["target"].all():
        assert not case["expected"][:, [1, 2]].any()


def test_cases_cover_the_shapes():
    built = [cases.case(name) for name in cases.NAMES]
    assert {c["rows"].shape[0] for c in built} == {1, 2, 63, 64, 65, 255, 256, 257, 700}
    assert {c["n_features"] for c in built} == {1, 3, 7, 66, 96}
    # the device walks two trees at a time: no pair, only the tree left over, one pair, one pair and a tree left over
    assert {0, 1, 2, 3} <= {c["forest"]["tree_offsets"].shape[0] - 1 for c in built}
    two = cases.case("two_trees")
    assert two["rows"].shape == (65, 3) and np.diff(two["forest"]["tree_offsets"]).max() <= 7   # depth 2 at most
    assert sum(not np.isnan(c["rows"]).any() for c in built if c["rows"].shape[0] > 2) == 1
    assert {("null" if c["target"] is None else "zeros" if not c["target"].any() else "ones" if c["target"].all()
             else "mixed") for c in built} == {"null", "zeros", "ones", "mixed"}
    assert any(c["forest"]["tree_offsets"].shape[0] == 1 for c in built)
    assert any(len(c["jobs"]) == 1 for c in built) and any(len(c["jobs"]) > 65535 for c in built)
    deep = cases.case("deep_tree")
    values = [job[2] for job in deep["jobs"] if job[0] == oracle.OVERRIDE]
    cut = values[3]
    assert np.isnan(values[0]) and values[1] == np.inf and values[2] == -np.inf and values[4] < cut
    assert values[4] == np.nextafter(cut, np.float32(-np.inf)) and cut in deep["forest"]["threshold"]
    # the value at the threshold and the one below it part ways
    at = [job[0] == oracle.OVERRIDE for job in deep["jobs"]].index(True)
    assert not np.array_equal(deep["expected"][at + 3], deep["expected"][at + 4])


# ---- validate_inspection -------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    from doppel_speller_amd import _lib

    def refuse():
        raise AssertionError("the library was called before the arguments were validated")
    monkeypatch.setattr(_lib, "lib", refuse)


ROWS = np.zeros((4, 7), np.float32)


@pytest.mark.parametrize("arguments, message", [
    (dict(rows=np.zeros((4, 6))), "rows must be a"),
    (dict(rows=np.zeros(7)), "rows must be a"),
    (dict(rows=np.zeros((4, 7), dtype=object)), "rows must be numbers"),
    (dict(rows=np.zeros((0, 7))), "n must be"),
    (dict(rows=None), "n must be"),
    (dict(rows=None, n=0), "n must be"),
    (dict(rows=None, n=(1 << 31) + 1), "n must be"),
    (dict(rows=None, n=2.0), "n must be"),
    (dict(target=[0, 1, 0]), "target must hold 4"),
    (dict(target=np.zeros((4, 1))), "target must hold 4"),
    (dict(target=[0, 1, 2, 0]), "target labels"),
    (dict(target=[0, 1, np.nan, 0]), "target labels"),
    (dict(n_repeats=0), "n_repeats"),
    (dict(n_repeats=1 << 16), "n_repeats"),
    (dict(n_repeats=2.0), "n_repeats"),
    (dict(n_repeats=True), "n_repeats"),
    (dict(seed=-1), "seed"),
    (dict(seed=1 << 63), "seed"),
    (dict(seed=1.5), "seed"),
    (dict(features=[0, 7]), "features"),
    (dict(features=[-1]), "features"),
    (dict(features=[1, 1]), "features must be unique"),
    (dict(features=[]), "features must not be empty"),
    (dict(features=3), "features must be a sequence"),
    (dict(features=["title_ratio", "no_such"]), "features 'no_such'"),
    (dict(feature=7), "feature"),
    (dict(feature="no_such"), "feature 'no_such'"),
    (dict(feature=1.0), "feature"),
    (dict(grid=[]), "grid must be 1-D and non-empty"),
    (dict(grid=[[1.0, 2.0]]), "grid must be 1-D and non-empty"),
    (dict(grid=["a"]), "grid must be an array of numbers"),
    (dict(n_grid=0), "n_grid"),
    (dict(threshold=0), "threshold"),
    (dict(threshold=1), "threshold"),
    (dict(threshold=float("nan")), "threshold"),
    (dict(threshold="high"), "threshold"),
    (dict(beta=0), "beta"),
    (dict(beta=float("inf")), "beta"),
    (dict(beta=None), "beta"),
])
def test_validate_inspection_refuses(no_library, arguments, message):
    import doppel_speller_amd as ds
    names = ("a", "b", "c", "d", "title_ratio", "e", "f")
    with pytest.raises(ValueError, match=message):
        ds.validate_inspection(7, **dict(dict(rows=ROWS, names=names), **arguments))


def test_validate_inspection_accepts(no_library):
    import doppel_speller_amd as ds
    names = ("a", "b", "c", "d", "title_ratio", "e", "f")
    v = ds.validate_inspection(7, rows=np.zeros((4, 7), np.int64), target=[0, 1, 1, 0], n_repeats=65535, seed=(1 << 63) - 1,
                               features=["title_ratio", 0], feature="title_ratio", grid=[np.nan, np.inf, 1], names=names)
    assert v["rows"].dtype == np.float32 and v["n"] == 4 and v["target"].dtype == np.float32
    assert v["features"].tolist() == [4, 0] and v["feature"] == 4 and v["grid"].dtype == np.float32
    v = ds.validate_inspection(7, n=1 << 31)
    assert v["features"].tolist() == list(range(7)) and v["rows"] is None and v["grid"] is None and v["target"] is None


def test_default_grid():
    import doppel_speller_amd as ds
    column = np.array([5, np.nan, 1, 3, 3, 2, np.nan, 4, 9], np.float32)
    for n_grid in (1, 2, 3, 4, 32):
        expected = oracle.quantile_grid(column, n_grid)
        assert ds.quantile_grid(column, n_grid).tobytes() == expected.tobytes()
    assert np.array_equal(oracle.quantile_grid(column, 3), np.array([1, 3, 9, np.nan], np.float32), equal_nan=True)
    assert ds.quantile_grid(np.array([np.nan, np.nan], np.float32), 4).tobytes() == np.array([np.nan], np.float32).tobytes()
    assert ds.quantile_grid(np.array([2.0, 2.0], np.float32), 4).tolist() == [2.0]


def test_results_are_derived_from_the_integers():
    import doppel_speller_amd as ds
    rng = np.random.RandomState(3)
    counters = rng.randint(0, 50, (1 + 3 * 4, 5)).astype(np.int64)
    counters[:, 4] = rng.randint(-(1 << 30), 1 << 30, counters.shape[0])
    counters[5:9] = counters[1:5]                                     # two features tie
    features = [6, 2, 4]
    got = ds.PermutationImportance(counters.view(np.uint64), 100, features, 4, 9, 0.9, 5.0)
    expected = oracle.permutation_importance(counters.view(np.uint64), 100, 3, 4, 5.0)
    assert got.baseline == expected["baseline"] and got.baseline_error == expected["baseline_error"]
    for key in ("error_matrix", "errors", "importance", "importance_std", "margin_shift"):
        assert getattr(got, key).dtype == expected[key].dtype and getattr(got, key).tobytes() == expected[key].tobytes()
    order = oracle.importance_order(features, expected["importance"])
    assert got.order().tolist() == order
    frame = got.frame(names=("a", "b", "c"))
    assert frame["feature"].tolist() == [features[s] for s in order]
    assert frame["name"].tolist() == [("a", "b", "c")[f] if f < 3 else f"f{f}" for f in frame["feature"]]
    assert frame["importance"].tolist() == sorted(expected["importance"], reverse=True)
    assert (got.features.tolist(), got.n_repeats, got.seed) == (features, 4, 9)
    dependence = ds.PartialDependence(counters.view(np.uint64), 100, 2, np.arange(12), 0.9)
    expected = oracle.partial_dependence(counters.view(np.uint64), 100)
    assert dependence.baseline_mean_margin == expected["baseline_mean_margin"]
    assert dependence.mean_margin.tobytes() == expected["mean_margin"].tobytes()
    assert dependence.positive_share.tobytes() == expected["positive_share"].tobytes()
    assert dependence.grid.dtype == np.float32


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_header_and_symbol_lists():
    from doppel_speller_amd import _lib
    from doppel_speller_amd import forest
    header = open(os.path.join(ROOT, "include", "doppel_amd.h")).read()
    assert re.search(r"int ds_forest_inspect_device\(ds_forest \*forest, const float \*d_rows, int64_t n, "
                     r"const float \*d_target,\s+const ds_inspect_job \*d_jobs, int32_t n_jobs, uint64_t seed, "
                     r"double threshold,\s+unsigned long long \*d_out, void \*stream\);", header)
    assert re.search(r"int ds_forest_inspect\(ds_forest \*forest, const float \*rows, int64_t n, const float \*target, "
                     r"const ds_inspect_job \*jobs,\s+int32_t n_jobs, uint64_t seed, double threshold, "
                     r"unsigned long long \*out\);", header)
    assert re.search(r"typedef struct ds_inspect_job \{\s+int32_t kind;\s+int32_t feature;\s+float value;\s+"
                     r"uint32_t repeat;\s+\} ds_inspect_job;", header)
    assert re.search(r"#define DS_INSPECT_PURPOSE_PERMUTE 6\b", header)
    for name, value in (("BASELINE", 0), ("PERMUTE", 1), ("OVERRIDE", 2), ("COUNTERS", 5)):
        assert re.search(rf"#define DS_INSPECT_{name} {value}\b", header)
    assert (forest.INSPECT_BASELINE, forest.INSPECT_PERMUTE, forest.INSPECT_OVERRIDE) == (0, 1, 2)
    assert forest.INSPECT_JOB.itemsize == 16 and forest.INSPECT_JOB.names == ("kind", "feature", "value", "repeat")
    assert [forest.INSPECT_JOB.fields[name][1] for name in forest.INSPECT_JOB.names] == [0, 4, 8, 12]
    assert {"ds_forest_inspect_device", "ds_forest_inspect"} <= set(_lib.EXPORTED_SYMBOLS)
    assert len(set(_lib.EXPORTED_SYMBOLS)) == len(_lib.EXPORTED_SYMBOLS)
    assert "ds_inspect.hip" in _lib._SOURCES and len(set(_lib._SOURCES)) == len(_lib._SOURCES)


def test_job_tables():
    from doppel_speller_amd import forest
    table = forest.permutation_jobs([4, 0], 3)
    assert [tuple(job) for job in table.tolist()] == [(k, f, 0.0, r) for k, f, v, r in oracle.permutation_jobs([4, 0], 3)]
    grid = np.array([1.5, np.nan, np.inf], np.float32)
    table = forest.dependence_jobs(2, grid)
    assert table["kind"].tolist() == [0, 2, 2, 2] and table["feature"].tolist() == [0, 2, 2, 2]
    assert table["value"][1:].tobytes() == grid.tobytes() and not table["repeat"].any()
    assert forest.inspection_jobs(oracle.dependence_jobs(2, grid)).tobytes() == table.tobytes()


@pytest.fixture(scope="module")
def library():
    import doppel_speller_amd as ds
    handle = ctypes.CDLL(ds.build_library())
    handle.ds_last_error.restype = ctypes.c_char_p
    return handle


def _p(array):
    return None if array is None else array.ctypes.data_as(ctypes.c_void_p)


def test_library_refuses_without_gpu(library):
    from doppel_speller_amd.forest import INSPECT_JOB
    rows = np.zeros((4, 7), np.float32)
    out = np.full((2, 5), 77, np.uint64)
    good = np.zeros(2, INSPECT_JOB)
    good[1] = (1, 3, 0.0, 2)

    def host(forest=None, rows_=rows, n=4, target=None, jobs=good, n_jobs=2, seed=1, threshold=0.9, out_=out):
        return library.ds_forest_inspect(forest, _p(rows_), ctypes.c_int64(n), _p(target), _p(jobs), ctypes.c_int32(n_jobs),
                                         ctypes.c_uint64(seed), ctypes.c_double(threshold), _p(out_))

    def device(forest=None, rows_=rows, n=4, target=None, jobs=good, n_jobs=2, seed=1, threshold=0.9, out_=out):
        return library.ds_forest_inspect_device(forest, _p(rows_), ctypes.c_int64(n), _p(target), _p(jobs),
                                                ctypes.c_int32(n_jobs), ctypes.c_uint64(seed), ctypes.c_double(threshold),
                                                _p(out_), None)

    def bad_job(*fields):
        jobs = good.copy()
        jobs[1] = fields
        return jobs

    for call, name in ((host, b"ds_forest_inspect:"), (device, b"ds_forest_inspect_device:")):
        for arguments, message in ((dict(n_jobs=-1), b"n_jobs = -1"), (dict(n=-1), b"n = -1"),
                                   (dict(n=(1 << 31) + 1), b"outside [0, 2^31]"), (dict(threshold=0.0), b"threshold"),
                                   (dict(threshold=1.0), b"threshold"), (dict(threshold=float("nan")), b"threshold"),
                                   (dict(), b"null forest")):
            assert call(**arguments) == -1, arguments
            error = library.ds_last_error()
            assert error.startswith(name) and message in error, (arguments, error)
    for arguments in (dict(jobs=None), dict(out_=None), dict(rows_=None)):
        assert host(**arguments) == -1 and b"ds_forest_inspect: null pointer" in library.ds_last_error(), arguments
    for jobs, message in ((bad_job(3, 0, 0.0, 0), b"unknown kind 3"), (bad_job(-1, 0, 0.0, 0), b"unknown kind -1"),
                          (bad_job(1, -1, 0.0, 0), b"feature -1 outside"), (bad_job(2, 96, 0.0, 0), b"feature 96 outside"),
                          (bad_job(1, 3, 0.0, 1 << 16), b"repeat 65536")):
        assert host(jobs=jobs) == -1 and message in library.ds_last_error(), library.ds_last_error()
    assert host(jobs=bad_job(0, 1000, 0.0, 1 << 20)) == -1 and b"null forest" in library.ds_last_error()   # a baseline's fields are not read
    assert (out == 77).all()


@pytest.mark.parametrize("change, message", [
    (dict(permutation_repeats=-1), "permutation_repeats"),
    (dict(permutation_repeats=2.0), "permutation_repeats"),
    (dict(permutation_repeats=True), "permutation_repeats"),
    (dict(permutation_repeats=1 << 16), "permutation_repeats"),
    (dict(permutation_repeats=2, permutation_seed=-1), "permutation_seed"),
    (dict(permutation_repeats=2, evaluation_fractions=dict(generated=0, negative=0, positive=0)),
     "permutation_repeats needs an evaluation set"),
])
def test_train_model_validates_permutation_arguments(no_library, change, message):
    import doppel_speller_amd as ds
    good = dict(truth_titles=["alpha beta", "gamma delta", "epsilon zeta"], truth_title_ids=[5, 6, 7],
                train_titles=["alpha bet", "unknown"], train_title_ids=[5, -1], top_n=2, sample_n=1)
    with pytest.raises(ValueError, match=message):
        ds.train_model(**dict(good, **change))


def test_model_methods_validate_before_the_library(no_library):
    """The methods hand their arguments to validate_inspection before anything else (no handle is needed for that)."""
    import doppel_speller_amd as ds
    model = ds.ForestModel.__new__(ds.ForestModel)
    model.n_features, model.handle = 66, None
    rows = np.zeros((3, 66), np.float32)
    for call, message in ((lambda: model.permutation_importance(rows, [0, 1]), "target must hold 3"),
                          (lambda: model.permutation_importance(rows, None, n_repeats=0), "n_repeats"),
                          (lambda: model.permutation_importance_device(None, 0, None), "n must be"),
                          (lambda: model.partial_dependence(rows, "no_such"), "feature 'no_such'"),
                          (lambda: model.partial_dependence(rows, None), "feature must be"),
                          (lambda: model.partial_dependence(rows, 0, grid=[]), "grid must be"),
                          (lambda: model.partial_dependence_device(None, 3, "title_ratio", None), "grid and feature"),
                          (lambda: model.partial_dependence_device(None, 3, 66, [1.0]), "feature")):
        with pytest.raises(ValueError, match=message):
            call()
