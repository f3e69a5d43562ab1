"""The contributions stage without a GPU: the yardsticks of contributions_cases.py against each other, the validation that
comes before any library call, the host helpers and the C ABI surface."""
import os
import re

import numpy as np
import pytest

import contributions_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# The largest |tree_shap - shapley_brute_force| over every entry of enumerable_cases(), divided by S = |base_margin| +
# the sum over the trees of max |leaf|: the gap between two independent float64 computations of the same sums, the
# rounding scale of the problem.  Measured on the CPU on 2026-10-18: 2.07e-16.
MEASURED_GAP = 2.1e-16
TOL = cc.TOL_FACTOR                      # the device tests' tolerance per entry, in units of S


@pytest.fixture(scope="module")
def cases():
    return cc.enumerable_cases()


def test_tree_shap_is_the_shapley_value_of_the_path_dependent_expectation(cases):
    worst = 0.0
    for name, forest, cover, rows in cases:
        offsets = forest["tree_offsets"]
        for t in range(offsets.shape[0] - 1):
            used = set(forest["feature"][offsets[t]:offsets[t + 1]].tolist()) - {-1}
            assert len(used) <= 8
        gap = float(np.abs(cc.tree_shap(forest, cover, rows) - cc.shapley_brute_force(forest, cover, rows)).max())
        print(f"{name}: gap / S = {gap / cc.forest_scale(forest):.3e}")
        worst = max(worst, gap / cc.forest_scale(forest))
    # the standing condition of the device tolerance, and the recorded constant as an upper bound of today's gap
    assert worst < TOL / 16
    assert worst <= MEASURED_GAP * 4


def test_the_cases_hold_what_they_are_for(cases):
    forest, rows = cases[0][1], cases[0][3]
    offsets = forest["tree_offsets"]
    sizes = np.diff(offsets)
    assert 1 in sizes and 3 in sizes                               # a single leaf, a stump

    def repeats(forest):
        """The largest number of splits on one feature along one path."""
        best = 0
        for t in range(forest["tree_offsets"].shape[0] - 1):
            begin = int(forest["tree_offsets"][t])
            stack = [(0, [])]
            while stack:
                node, seen = stack.pop()
                f = int(forest["feature"][begin + node])
                if f < 0:
                    best = max([best] + [seen.count(x) for x in seen])
                    continue
                stack += [(int(forest["yes"][begin + node]), seen + [f]), (int(forest["no"][begin + node]), seen + [f])]
        return best
    assert repeats(forest) == 3 and repeats(cases[2][1]) >= 3
    inner = forest["feature"] >= 0
    assert (forest["missing"][inner] == forest["yes"][inner]).any() and (forest["missing"][inner] == forest["no"][inner]).any()
    assert np.isnan(rows).any()
    covers = cases[1][2][forest["feature"] < 0]
    assert covers.min() == 1.0 and covers.max() == 1e6


def test_saabas_equals_tree_shap_on_stumps_and_both_are_locally_accurate(cases):
    rng = np.random.RandomState(3)
    stumps = cc.from_trees([cc.tree([(int(rng.randint(5)), float(rng.choice([20.0, 50.0, 65.0])), 1, 2, 1 + int(rng.rand() < 0.5)),
                                     float(rng.normal()), float(rng.normal())]) for _ in range(20)], base_margin=0.7)
    rows = cc.small_rows(rng, 50, 5)
    cover = cc.additive_cover(stumps, rng.uniform(1, 30, stumps["feature"].shape[0]))
    exact, approximate = cc.tree_shap(stumps, cover, rows), cc.saabas(stumps, cover, rows)
    assert np.abs(exact - approximate).max() <= 1e-14 * cc.forest_scale(stumps)
    for name, forest, cover, rows in cases + [("stumps", stumps, cover, rows)]:
        margins = cc.margins64(forest, rows)
        for method in (cc.tree_shap, cc.saabas):
            assert np.abs(method(forest, cover, rows).sum(axis=1) - margins).max() <= 1e-13 * cc.forest_scale(forest)


def test_node_counts_known_answer():
    forest = cc.from_trees([cc.tree([(0, 50.0, 1, 2, 2), 0.1, (1, 20.0, 3, 4, 3), 0.2, 0.3])])
    rows = np.array([[10, 0], [np.nan, 10], [60, np.nan], [60, 30], [50, 20]], np.float32)
    assert cc.node_counts(forest, rows).tolist() == [5, 1, 4, 2, 2]


@pytest.fixture
def no_library(monkeypatch):
    from doppel_speller_amd import _lib

    def refuse():
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "lib", refuse)


def test_validate_cover(no_library):
    from doppel_speller_amd import validate_cover
    good = validate_cover([1, 2.5, 3], 3)
    assert good.dtype == np.float64 and good.tolist() == [1.0, 2.5, 3.0]
    for cover, message in (([1, 2], "shape"), ([[1, 2, 3]], "shape"), ([1, np.nan, 3], r"cover\[1\] is not finite"),
                           ([1, 2, np.inf], r"cover\[2\] is not finite"), ([1, 0, 3], r"cover\[1\] = 0.0 is not above 0"),
                           ([-1, 2, 3], r"cover\[0\]"), (["a", "b", "c"], "numbers")):
        with pytest.raises(ValueError, match=message):
            validate_cover(cover, 3)


def test_zero_cover_is_refused_by_name_and_a_prior_keeps_the_cover_additive(no_library):
    from doppel_speller_amd.forest import ForestModel, cover_from_counts
    forest = cc.awkward_forest()
    rows = cc.small_rows(np.random.RandomState(2), 3, 4)
    counts = cc.node_counts(forest, rows)
    at = int(np.flatnonzero(counts == 0)[0])
    tree = int(np.searchsorted(forest["tree_offsets"], at, side="right") - 1)
    with pytest.raises(ValueError, match=rf"no row reached node {at - forest['tree_offsets'][tree]} of tree {tree} "):
        cover_from_counts(counts, forest)
    with pytest.raises(ValueError, match="prior"):
        cover_from_counts(counts, forest, prior=-1.0)
    cover = cover_from_counts(counts, forest, prior=0.25)
    assert (cover > 0).all()
    inner = np.flatnonzero(forest["feature"] >= 0)
    begin = forest["tree_offsets"][np.searchsorted(forest["tree_offsets"], inner, side="right") - 1]
    assert np.array_equal(cover[inner], cover[begin + forest["yes"][inner]] + cover[begin + forest["no"][inner]])
    leaves = forest["feature"] < 0
    assert np.array_equal(cover[leaves], counts[leaves] + 0.25)
    full = cc.node_counts(forest, cc.small_rows(np.random.RandomState(2), 400, 4))
    assert np.array_equal(cover_from_counts(full, forest), full.astype(np.float64))
    # the model's methods reach those checks before the library
    model = ForestModel.__new__(ForestModel)
    model.arrays, model.n_features, model.cover, model.handle, model.device = forest, 4, None, None, 0
    with pytest.raises(ValueError, match="prior"):
        model.fit_cover(rows, prior=float("nan"))
    with pytest.raises(ValueError, match="shape"):
        model.set_cover(np.ones(3))


def test_explain_needs_a_cover_before_any_library_call(no_library):
    from doppel_speller_amd.prediction import Prediction

    class Model:
        cover = None
    p = Prediction.__new__(Prediction)
    p.model = Model()
    with pytest.raises(ValueError, match="no cover"):
        p.explain(["some title"])


def test_xgboost_cover_reads_sum_hessian_in_node_order(no_library):
    from doppel_speller_amd.forest import ForestModel
    trees = [dict(left_children=[1, -1, -1], right_children=[2, -1, -1], split_indices=[3, 0, 0],
                  split_conditions=[0.5, 0.1, -0.2], default_left=[1, 0, 0], sum_hessian=[10.0, 4.0, 6.0]),
             dict(left_children=[-1], right_children=[-1], split_indices=[0], split_conditions=[0.3], default_left=[0],
                  sum_hessian=[10.0])]
    model = {"learner": {"gradient_booster": {"model": {"trees": trees}}, "learner_model_param": {"base_score": "0.5"}}}
    assert ForestModel.xgboost_cover(model).tolist() == [10.0, 4.0, 6.0, 10.0]
    assert ForestModel.xgboost_cover(model, ntree_limit=1).tolist() == [10.0, 4.0, 6.0]
    arrays = ForestModel.parse_xgboost_model_json(model)
    assert arrays["feature"].shape[0] == 4 and sorted(arrays) == sorted(
        ["feature", "threshold", "yes", "no", "missing", "tree_offsets", "base_margin"])


def test_top_contributions_breaks_ties_by_the_lower_index():
    from doppel_speller_amd import top_contributions
    values = np.array([[0.5, -2.0, 2.0, 0.0, -0.5], [0.0, 0.0, 0.0, 0.0, 0.0]])
    index, value = top_contributions(values, n=3)
    assert index.tolist() == [[1, 2, 0], [0, 1, 2]] and value.tolist() == [[-2.0, 2.0, 0.5], [0.0, 0.0, 0.0]]
    index, value = top_contributions(values, n=9)
    assert index.shape == (2, 5) and index[0].tolist() == [1, 2, 0, 4, 3]
    for bad in (0, True, 1.5):
        with pytest.raises(ValueError):
            top_contributions(values, n=bad)


def test_feature_names():
    import doppel_speller_amd as ds
    assert len(ds.FEATURE_NAMES) == ds.FEATURES_COUNT == 66 and len(set(ds.FEATURE_NAMES)) == 66
    assert isinstance(ds.FEATURE_NAMES, tuple) and all(isinstance(name, str) and name for name in ds.FEATURE_NAMES)
    assert ds.EXPLAIN_COLUMNS == ("test_index", "match_row", "title_id", "probability", "margin", "bias", "stage",
                                  "answer_row")


def test_header_declares_what_the_binding_calls():
    from doppel_speller_amd import _lib
    header = open(os.path.join(ROOT, "include", "doppel_amd.h")).read()
    flat = re.sub(r"\s+", " ", header)
    for declaration in (
            "int ds_forest_cover_device(ds_forest *forest, const float *d_rows, int64_t n, void *stream);",
            "int ds_forest_cover_set(ds_forest *forest, const double *cover);",
            "int ds_forest_cover_read(ds_forest *forest, double *cover);",
            "int ds_forest_cover_clear(ds_forest *forest);",
            "int ds_forest_option(ds_forest *forest, const char *name, int64_t value);",
            "int ds_forest_contributions_device(ds_forest *forest, const float *d_rows, int64_t n, double *d_out, "
            "int approximate, void *stream);",
            "int ds_forest_contributions(ds_forest *forest, const float *rows, int64_t n, double *out, int approximate);"):
        assert declaration in flat, declaration
    assert {"ds_forest_cover_device", "ds_forest_cover_set", "ds_forest_cover_read", "ds_forest_cover_clear",
            "ds_forest_option", "ds_forest_contributions_device", "ds_forest_contributions",
            "ds_best_pairs_device"} <= set(_lib.EXPORTED_SYMBOLS)
    assert "ds_contributions.hip" in _lib._SOURCES


def test_library_builds_and_refuses_bad_arguments_without_a_device():
    import ctypes
    import doppel_speller_amd as ds
    library = ctypes.CDLL(ds.build_library())               # hipcc --offload-arch=gfx950
    library.ds_last_error.restype = ctypes.c_char_p
    for name in ("ds_forest_cover_device", "ds_forest_contributions_device", "ds_best_pairs_device"):
        assert hasattr(library, name)
    assert library.ds_forest_contributions_device(None, None, ctypes.c_int64(0), None, 0, None) == -1
    assert library.ds_forest_cover_set(None, None) == -1 and library.ds_forest_option(None, b"max_blocks", 0) == -1
    assert library.ds_best_pairs_device(None, None, ctypes.c_int64(3), 0, None, None, None, None, None) == -1
    assert b"ds_best_pairs_device" in library.ds_last_error()
