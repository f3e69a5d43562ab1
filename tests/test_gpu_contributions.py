"""Node cover and per-feature contributions on the device (csrc/ds_contributions.hip) against the NumPy yardsticks of
contributions_cases.py: exact counts, TreeSHAP and Saabas within TOL = 1e-10 * S per entry (S = |base_margin| + the sum
over the trees of max |leaf|; two independent float64 computations of these sums differ by 2e-16 * S,
test_contributions_cpu.MEASURED_GAP), local accuracy, determinism, limits."""
import os

import numpy as np
import pytest

import contributions_cases as cc

pytestmark = pytest.mark.gpu


def _model(forest, n_features):
    from doppel_speller_amd.forest import ForestModel
    return ForestModel(forest["feature"], forest["threshold"], forest["yes"], forest["no"], forest["missing"],
                       forest["tree_offsets"], n_features, forest["base_margin"])


def _dump_forest(seed, n_trees, n_features, depth):
    from doppel_speller_amd.forest import ForestModel
    return ForestModel.parse_xgboost_dump(cc.random_dump(seed, n_trees=n_trees, n_features=n_features, depth=depth))


def _nan_rows(seed, n, n_features):
    """Rows of random_rows with a tenth of the values NaN."""
    rng = np.random.RandomState(seed)
    rows = rng.uniform(0, 100, (n, n_features)).astype(np.float32)
    rows[:, :min(6, n_features)] = rng.randint(0, 100, (n, min(6, n_features)))
    rows[rng.rand(n, n_features) < 0.1] = np.nan
    return rows


@pytest.fixture(scope="module")
def sixty():
    """The 60-tree depth-6 model on 66 features with a counted cover + 1, 1,000 rows with NaNs, and the yardsticks."""
    forest = _dump_forest(31, 60, 66, 6)
    model = _model(forest, 66)
    background = _nan_rows(32, 5000, 66)
    cover = model.fit_cover(background, prior=1.0)
    rows = _nan_rows(33, 1000, 66)
    return dict(forest=forest, model=model, cover=cover, rows=rows, background=background,
                shap=cc.tree_shap(forest, cover, rows), saabas=cc.saabas(forest, cover, rows))


# ---- cover -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def counting():
    forest = _dump_forest(41, 60, 66, 6)
    rows = _nan_rows(42, 70000, 66)
    return dict(forest=forest, model=_model(forest, 66), rows=rows)


@pytest.mark.parametrize("n", [1, 255, 257, 70000])
@pytest.mark.parametrize("max_blocks", [0, 2])
def test_cover_counts_are_exact(counting, n, max_blocks):
    from doppel_speller_amd import _lib
    model, rows = counting["model"], counting["rows"][:n]
    model.option("max_blocks", max_blocks)
    try:
        d_rows = _lib.DeviceArray.from_host(rows)
        counts = model.count_cover_device(d_rows, n)
    finally:
        model.option("max_blocks", 0)
    expected = cc.node_counts(counting["forest"], rows)
    assert counts.dtype == np.float64 and np.array_equal(counts, expected.astype(np.float64))
    roots = counting["forest"]["tree_offsets"][:-1]
    assert (counts[roots] == n).all()


def test_cover_calls_accumulate_and_round_trip(counting, tmp_path):
    from doppel_speller_amd import DoppelError, _lib
    from doppel_speller_amd.forest import ForestModel
    forest, rows = counting["forest"], counting["rows"]
    model = _model(forest, 66)
    assert model.cover is None
    with pytest.raises(DoppelError, match="no cover"):
        model.read_cover()
    first, second = _lib.DeviceArray.from_host(rows[:300]), _lib.DeviceArray.from_host(rows[300:1000])
    model.count_cover_device(first, 300)
    both = model.count_cover_device(second, 700, accumulate=True)
    assert np.array_equal(both, cc.node_counts(forest, rows[:1000]).astype(np.float64))
    again = model.count_cover_device(second, 700)                 # a fresh count starts from zero
    assert np.array_equal(again, cc.node_counts(forest, rows[300:1000]).astype(np.float64))
    # set / read / clear
    given = np.random.RandomState(1).uniform(0.5, 9.0, model.n_nodes)
    model.set_cover(given)
    assert np.array_equal(model.read_cover(), given) and np.array_equal(model.cover, given)
    model.set_cover(None)
    assert model.cover is None
    with pytest.raises(DoppelError, match="no cover"):
        model.read_cover()
    with pytest.raises(ValueError, match="not above 0"):
        model.set_cover(np.zeros(model.n_nodes))
    # a node no row reached is refused by name unless a prior is given; the prior keeps the cover additive
    with pytest.raises(ValueError, match="no row reached node"):
        model.fit_cover(rows[:1])
    assert model.cover is None
    cover = model.fit_cover(rows[:1], prior=0.5)
    inner = np.flatnonzero(forest["feature"] >= 0)
    tree_of = np.searchsorted(forest["tree_offsets"], inner, side="right") - 1
    begin = forest["tree_offsets"][tree_of]
    assert np.array_equal(cover[inner], cover[begin + forest["yes"][inner]] + cover[begin + forest["no"][inner]])
    # save / load keep the cover; a model without one saves the keys of before
    with_cover, without = str(tmp_path / "with.npz"), str(tmp_path / "without.npz")
    model.save(with_cover)
    loaded = ForestModel.load(with_cover)
    assert np.array_equal(loaded.cover, cover) and np.array_equal(loaded.read_cover(), cover)
    model.set_cover(None)
    model.save(without)
    keys = {"feature", "threshold", "yes", "no", "missing", "tree_offsets", "base_margin", "n_features"}
    assert set(np.load(without).files) == keys and set(np.load(with_cover).files) == keys | {"cover"}
    assert ForestModel.load(without).cover is None


# ---- contributions -----------------------------------------------------------------------------------------------------
def _check(model, forest, cover, rows, approximate=False, expected=None):
    """predict_contributions within TOL of the yardstick, locally accurate, and exactly 0.0 for unused features."""
    got = model.predict_contributions(rows, approximate=approximate)
    if expected is None:
        expected = (cc.saabas if approximate else cc.tree_shap)(forest, cover, rows)
    tolerance = cc.TOL_FACTOR * cc.forest_scale(forest)
    worst = float(np.abs(got - expected).max()) if rows.shape[0] else 0.0
    print(f"max |difference| = {worst:.3e}, TOL = {tolerance:.3e}")
    assert got.shape == expected.shape and got.dtype == np.float64
    assert worst <= tolerance
    # local accuracy against the forest kernel's float32 margin: T * 2^-24 * sum of max |leaf| (sequential float32 sum)
    n_trees = forest["tree_offsets"].shape[0] - 1
    margins = model.predict(rows, output_margin=True).astype(np.float64)
    bound = n_trees * 2.0 ** -24 * cc.leaf_sum_bound(forest)
    gap = float(np.abs(got.sum(axis=1) - margins).max()) if rows.shape[0] else 0.0
    print(f"local accuracy gap = {gap:.3e}, bound = {bound:.3e}")
    assert gap <= bound
    unused = np.setdiff1d(np.arange(rows.shape[1]), forest["feature"][forest["feature"] >= 0])
    assert (got[:, unused] == 0.0).all() and not np.signbit(got[:, unused]).any()
    return got


def test_one_stump_one_row():
    forest = cc.from_trees([cc.tree([(0, 50.0, 1, 2, 1), 0.25, -0.5])], base_margin=0.1)
    model = _model(forest, 1)
    cover = np.array([10.0, 3.0, 7.0])
    model.set_cover(cover)
    got = _check(model, forest, cover, np.array([[20.0]], np.float32))
    mean = 0.3 * np.float64(np.float32(0.25)) + 0.7 * -0.5
    assert abs(got[0, 1] - (np.float64(np.float32(0.1)) + mean)) < 1e-15 and abs(got[0, 0] - (0.25 - mean)) < 1e-15


def test_every_path_repeats_features():
    rng = np.random.RandomState(5)
    forest = cc.from_trees([cc.random_tree(rng, [0, 1], 6, leaf_chance=0.1) for _ in range(3)], base_margin=0.3)
    model = _model(forest, 2)
    rows = cc.small_rows(rng, 300, 2)
    cover = model.fit_cover(cc.small_rows(rng, 2000, 2), prior=1.0)
    _check(model, forest, cover, rows)
    _check(model, forest, cover, rows, approximate=True)


def test_sixty_trees_of_depth_six(sixty):
    _check(sixty["model"], sixty["forest"], sixty["cover"], sixty["rows"], expected=sixty["shap"])


def test_sixty_trees_of_depth_six_approximate(sixty):
    _check(sixty["model"], sixty["forest"], sixty["cover"], sixty["rows"], approximate=True, expected=sixty["saabas"])


def test_three_hundred_trees_of_depth_four():
    forest = _dump_forest(51, 300, 66, 4)
    model = _model(forest, 66)
    cover = model.fit_cover(_nan_rows(52, 3000, 66), prior=1.0)
    _check(model, forest, cover, _nan_rows(53, 257, 66))


def test_awkward_trees_and_unequal_covers():
    """The enumerable cases of the CPU test (stump, single leaf, repeats, empty intervals, covers of 1 against 10^6).
    The cover kernel counts their rows first: the single leaf is a tree whose walk takes no step."""
    from doppel_speller_amd import _lib
    for name, forest, cover, rows in cc.enumerable_cases():
        model = _model(forest, rows.shape[1])
        d_rows = _lib.DeviceArray.from_host(rows)
        counted = model.count_cover_device(d_rows, rows.shape[0])
        d_rows.free()
        assert np.array_equal(counted, cc.node_counts(forest, rows).astype(np.float64)), name
        model.set_cover(cover)
        _check(model, forest, cover, rows)
        _check(model, forest, cover, rows, approximate=True)


@pytest.mark.parametrize("n_features", [1, 47, 48, 96])
def test_every_lds_layout(n_features):
    forest = _dump_forest(60 + n_features, 12, n_features, 5)
    model = _model(forest, n_features)
    cover = model.fit_cover(cc.random_rows(61, 1500, n_features), prior=1.0)
    rows = cc.random_rows(62, 130, n_features)
    _check(model, forest, cover, rows)
    _check(model, forest, cover, rows, approximate=True)


def test_depth_limit():
    from doppel_speller_amd import DoppelError
    rng = np.random.RandomState(9)
    deep = cc.from_trees([cc.tree([(0, 50.0, 1, 2, 1), 0.1, 0.2]), cc.chain_tree(16, 20, rng)])
    model = _model(deep, 20)
    rows = cc.small_rows(rng, 70, 20)
    cover = model.fit_cover(cc.small_rows(rng, 500, 20), prior=1.0)
    _check(model, deep, cover, rows)
    too_deep = cc.from_trees([cc.tree([(0, 50.0, 1, 2, 1), 0.1, 0.2]), cc.chain_tree(17, 20, rng)])
    model = _model(too_deep, 20)                              # the limit is not ds_forest_create's
    model.predict(rows)
    model.fit_cover(cc.small_rows(rng, 500, 20), prior=1.0)
    with pytest.raises(DoppelError, match=r"tree 1 is 17 splits deep.*status -1"):
        model.predict_contributions(rows)


def test_deterministic_whatever_the_grid(sixty):
    model, rows = sixty["model"], sixty["rows"][:300]
    for approximate in (False, True):
        default = model.predict_contributions(rows, approximate=approximate)
        assert np.array_equal(default, model.predict_contributions(rows, approximate=approximate))
        for max_blocks in (1, 3):
            model.option("max_blocks", max_blocks)
            try:
                capped = model.predict_contributions(rows, approximate=approximate)
            finally:
                model.option("max_blocks", 0)
            assert np.array_equal(capped.view(np.uint64), default.view(np.uint64))


def test_no_cover_and_no_rows(sixty):
    from doppel_speller_amd import DoppelError
    bare = _model(sixty["forest"], 66)
    with pytest.raises(DoppelError, match="no cover"):
        bare.predict_contributions(sixty["rows"][:4])
    empty = sixty["model"].predict_contributions(np.zeros((0, 66), np.float32))
    assert empty.shape == (0, 67)
    with pytest.raises(DoppelError, match="max_blocks"):
        bare.option("max_blocks", -1)
