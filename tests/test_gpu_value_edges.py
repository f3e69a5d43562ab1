"""Every place on the device that maps a raw float32 value to a tree branch, on hostile values (value_cases.py;
DESIGN.md section 9, "Order of values"): the bin kernel, the trainer's bin walk against the forest's float walk, the
seed kernel, prediction, cover, refresh, inspection and TreeSHAP, on denormals, signed zeros, infinities, NaN and
values one float32 step from a cut.  Bit for bit or integer-equal throughout, except the contributions (the tolerance
of test_gpu_contributions.py) and the probabilities (rtol 3e-7, as in test_gpu_forest.py).  test_value_cases_cpu.py
proves that the references used here agree with each other on these inputs."""
import time

import numpy as np
import pytest

import forest_continue_oracle as continued
import forest_inspect_oracle as inspected
import forest_train_oracle as trained
import inspect_cases
import value_cases as vc
from test_forest_cpu import random_rows
from test_gpu_continue import continue_against_the_oracle
from test_gpu_contributions import _check as check_contributions
from test_gpu_refresh import against_oracle as refresh_against_oracle
from test_gpu_trainer import check_rounds

pytestmark = pytest.mark.gpu

FORESTS = ["hostile_forest", "trained"]


@pytest.fixture(autouse=True)
def wall_time(request):
    started = time.perf_counter()
    yield
    print(f"{request.node.name}: {time.perf_counter() - started:.2f} s")


def bits(a):
    return np.asarray(a).tobytes()


def begin(h, **more):
    """A trainer on the crafted part of a hostile matrix with the extra rows as its evaluation set (value_cases.TRAINED)."""
    import doppel_speller_amd as ds
    q = vc.TRAINED
    return ds.ForestTrainer().begin(h.train, h.y, h.extra, h.extra_y, max_depth=q["max_depth"], eta=q["eta"],
                                    min_child_weight=q["min_child_weight"], reg_lambda=q["reg_lambda"],
                                    max_bin=h.max_bin, **more)


@pytest.fixture(scope="module")
def grown():
    """The model the device grows on the crafted part at max_bin 256 in twelve rounds, and its training margins."""
    trainer = begin(vc.hostile_matrix(256))
    for _ in range(vc.TRAINED["rounds"]):
        trainer.step()
    out = dict(model=trainer.model(), margins=trainer.margins(), eval_margins=trainer.eval_margins())
    trainer.close()
    return out


@pytest.fixture(scope="module")
def forests(grown):
    """name -> (ForestModel, its flat arrays); the rows are those of hostile_matrix(256)."""
    import doppel_speller_amd as ds
    hostile = vc.hostile_forest(0)
    model = ds.ForestModel(hostile["feature"], hostile["threshold"], hostile["yes"], hostile["no"], hostile["missing"],
                           hostile["tree_offsets"], 22, hostile["base_margin"])
    return {"hostile_forest": (model, hostile), "trained": (grown["model"], grown["model"].arrays)}


# ---- bins ---------------------------------------------------------------------------------------------------------------
def device_bins(x, max_bin, form):
    """(bins, cuts, cut_offsets) of a trainer begun on x through the host entry or begin_device."""
    import doppel_speller_amd as ds
    y = np.zeros(x.shape[0], np.float32)
    trainer = ds.ForestTrainer()
    if form == "device":
        d_x = ds._lib.DeviceArray.from_host(x)
        trainer.begin_device(d_x, x.shape[0], y, max_bin=max_bin)
        d_x.free()
    else:
        trainer.begin(x, y, max_bin=max_bin)
    out = trainer.bins(), trainer.cuts, trainer.cut_offsets
    trainer.close()
    return out


def check_bins(x, max_bin, form):
    x = np.ascontiguousarray(x, dtype=np.float32)
    per_feature = trained.cuts(x, max_bin)
    bins, cuts, offsets = device_bins(x, max_bin, form)
    assert bits(cuts) == bits(np.concatenate(per_feature).astype(np.float32))
    assert offsets.tolist() == [0] + np.cumsum([c.shape[0] for c in per_feature]).tolist()
    expected = trained.bins(x, per_feature)
    assert bins.dtype == np.uint8 and bins.shape == expected.shape and bits(bins) == bits(expected)
    return per_feature


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("max_bin", [256, 16, 2])
def test_bins_of_the_crafted_columns(max_bin, form):
    check_bins(vc.hostile_matrix(max_bin).train, max_bin, form)


@pytest.mark.parametrize("form", ["host", "device"])
def test_bins_with_every_entry_of_the_cut_table_read(form):
    per_feature = check_bins(vc.full_table_matrix(), 256, form)
    assert [c.shape[0] for c in per_feature] == [254] * 96


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("nf", [1, 96])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_bins_around_a_row_tile(n, nf, form):
    """kBinTileRows = 64: one row, a tile less one, a whole tile, one more, two tiles and one row; column 0 is denormal."""
    check_bins(vc.full_table_matrix()[:n, :nf], 256, form)


# ---- the bin walk is the float walk ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_bin", [256, 16])
def test_training_on_bins_and_predicting_on_floats_reach_the_same_leaves(max_bin):
    """check_rounds compares every tree with the oracle's and, bit for bit, the trainer's margins (rows routed by their
    bins) with ForestModel.predict on the raw rows (routed by float comparison): the crafted rows, and the rows on, one
    step below and one step above every cut as the evaluation set."""
    h = vc.hostile_matrix(max_bin)
    q = vc.TRAINED
    trainer = begin(h)
    check_rounds(trainer, h.train, h.y, h.extra, h.extra_y, q["rounds"], q["max_depth"], q["eta"],
                 q["min_child_weight"], q["reg_lambda"], max_bin)
    model = trainer.model()
    denormal, zero, infinite = vc.threshold_census(model.arrays)
    print(f"max_bin {max_bin}: the device trees hold {denormal} denormal thresholds, {zero} equal to 0.0, {infinite} "
          f"equal to +inf (the oracle's own trees: {vc.threshold_census(vc.oracle_trained(max_bin))})")
    assert model.n_trees == q["rounds"] and denormal >= 20 and zero >= 5 and infinite >= 5
    leaves, _ = vc.key_walk(model.arrays, h.rows)
    sums = np.float32(0.0) + vc.leaf_sums(model.arrays, leaves)
    assert bits(trainer.margins()) == bits(sums[:h.n_train]) and bits(trainer.eval_margins()) == bits(sums[h.n_train:])
    trainer.close()
    model.close()


def test_a_trainer_seeded_with_the_model_starts_from_its_leaves(grown):
    """ds_train_seed_kernel walks the raw rows: its margins are the oracle's, and three more rounds are the oracle's."""
    h = vc.hostile_matrix(256)
    q = vc.TRAINED
    init = grown["model"]
    arrays = {key: init.arrays[key] for key in init.arrays}
    parameters = dict(max_depth=q["max_depth"], eta=q["eta"], min_child_weight=q["min_child_weight"],
                      reg_lambda=q["reg_lambda"])
    want = continued.train(h.train, h.y, 0, arrays, h.extra, h.extra_y, **parameters)
    trainer = begin(h, init_model=init)
    assert bits(trainer.margins()) == bits(want["margins"]) == bits(grown["margins"])
    assert bits(trainer.eval_margins()) == bits(want["eval_margins"]) == bits(grown["eval_margins"])
    assert trainer.initial_error == trained.custom_error(init.predict(h.extra), h.extra_y)
    booster = continued.ContinueBooster(h.train, h.y, arrays, parameters)
    continue_against_the_oracle(trainer, booster, h.train, h.extra, h.extra_y, 3, continued.leaf_sums(arrays, h.extra))
    assert trainer.model().n_trees == q["rounds"] + 3
    trainer.close()


# ---- the raw-value walkers ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FORESTS)
def test_predict_equals_the_c_oracle(oracle, forests, name):
    model, arrays = forests[name]
    rows = vc.hostile_matrix(256).rows
    margins, probabilities = oracle.forest_predict(arrays, rows)
    assert bits(model.predict(rows, output_margin=True)) == bits(margins)
    assert np.allclose(model.predict(rows), probabilities, rtol=3e-7, atol=0)


@pytest.mark.parametrize("name", FORESTS)
def test_cover_counts_equal_the_key_walk(forests, name):
    from doppel_speller_amd import _lib
    model, arrays = forests[name]
    rows = vc.hostile_matrix(256).rows
    _, counts = vc.key_walk(arrays, rows)
    d_rows = _lib.DeviceArray.from_host(rows)
    try:
        counted = model.count_cover_device(d_rows, rows.shape[0])
        assert counted.dtype == np.float64 and np.array_equal(counted, counts.astype(np.float64))
        assert np.array_equal(model.read_cover(), counts.astype(np.float64))
    finally:
        d_rows.free()
        model.set_cover(None)


@pytest.mark.parametrize("name", FORESTS)
def test_refresh_sums_and_leaves_equal_the_oracle(forests, name):
    model, _ = forests[name]
    h = vc.hostile_matrix(256)
    result, want = refresh_against_oracle(model, h.rows, vc.labels(h.rows, h.names))
    leaves = model.arrays["feature"] < 0
    assert np.count_nonzero(want["leaves"][leaves] != model.arrays["threshold"][leaves]) > leaves.sum() // 2
    result.model.close()


@pytest.mark.parametrize("column", ["denormals", "infinities"])
@pytest.mark.parametrize("name", FORESTS)
def test_partial_dependence_on_every_threshold_and_its_neighbours(forests, name, column):
    model, arrays = forests[name]
    h = vc.hostile_matrix(256)
    rows, target, feature = h.rows, vc.labels(h.rows, h.names), h.names.index(column)
    grid = vc.inspection_grid(arrays, feature)
    assert grid.shape[0] >= 5 + 3 and np.isnan(grid).sum() == 1         # the forest does split on the column
    # ds_inspect.hip walks two trees at a time and an odd last tree on its own: 13 trees run both walks, 12 the first
    assert (arrays["tree_offsets"].shape[0] - 1) % 2 == (name == "hostile_forest")
    result = model.partial_dependence(rows, feature, grid=grid, target=target)
    counters, gap = inspected.inspect(arrays, rows, target, inspected.dependence_jobs(feature, grid), 0)
    assert gap >= inspect_cases.PROBABILITY_GAP
    expected = inspected.partial_dependence(counters, rows.shape[0])
    assert bits(result.grid) == bits(grid) and bits(result.counters) == bits(counters)
    assert result.baseline_mean_margin == expected["baseline_mean_margin"]
    assert bits(result.mean_margin) == bits(expected["mean_margin"])
    assert bits(result.positive_share) == bits(expected["positive_share"])
    assert len(np.unique(result.mean_margin)) >= 3


@pytest.mark.parametrize("name", FORESTS)
def test_permutation_importance_of_a_denormal_and_an_infinite_column(forests, name):
    model, arrays = forests[name]
    h = vc.hostile_matrix(256)
    rows, target = h.rows, vc.labels(h.rows, h.names)
    features = [h.names.index("denormals"), h.names.index("infinities")]
    result = model.permutation_importance(rows, target, n_repeats=2, seed=77, features=features)
    counters, gap = inspected.inspect(arrays, rows, target, inspected.permutation_jobs(features, 2), 77)
    assert gap >= inspect_cases.PROBABILITY_GAP
    expected = inspected.permutation_importance(counters, rows.shape[0], 2, 2)
    assert bits(result.counters) == bits(counters)
    for key in ("error_matrix", "errors", "importance", "importance_std", "margin_shift"):
        assert bits(getattr(result, key)) == bits(expected[key]), key
    assert (result.counters[1:] != result.counters[0]).any(axis=1).all()      # every shuffle moved some row


# ---- TreeSHAP: merged bounds instead of a walk ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FORESTS)
def test_contributions_on_merged_bounds(forests, name):
    """predict_contributions, exact and approximate, with the cover counted from the same rows (+ 1 per leaf: the
    `yes` child of a NaN or -inf threshold is reached by no value), within test_gpu_contributions.py's tolerances,
    local accuracy against the device margin included."""
    model, arrays = forests[name]
    rows = vc.hostile_matrix(256).rows
    # elements merged from two or more splits where the forest has them; the grown trees meet no feature twice on a path
    merged = [b for b in vc.merged_bounds(arrays) if b[3] >= (2 if name == "hostile_forest" else 1)]
    on_lo = sum(1 for f, lo, _, _ in merged if lo is not None and (vc.key(rows[:, f]) == vc.key(np.float32(lo))).any())
    on_hi = sum(1 for f, _, hi, _ in merged if hi is not None and (vc.key(rows[:, f]) == vc.key(np.float32(hi))).any())
    print(f"{len(merged)} path elements; with a compared row exactly on lo: {on_lo}, exactly on hi: {on_hi}")
    assert on_lo >= 50 and on_hi >= 50
    try:
        cover = model.fit_cover(rows, prior=1.0)
        check_contributions(model, arrays, cover, rows)
        check_contributions(model, arrays, cover, rows, approximate=True)
    finally:
        model.set_cover(None)


# ---- a row's leaf does not depend on its neighbours ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", FORESTS)
def test_hostile_rows_alone_and_among_a_hundred_thousand_others(forests, name):
    model, _ = forests[name]
    rows = vc.hostile_matrix(256).rows
    others = random_rows(5, 100000, 22)
    mine = np.zeros(rows.shape[0] + others.shape[0], bool)
    mine[np.random.RandomState(6).choice(mine.shape[0], rows.shape[0], replace=False)] = True
    mixed = np.empty((mine.shape[0], 22), np.float32)
    mixed[mine], mixed[~mine] = rows, others
    for output_margin in (True, False):
        alone = model.predict(rows, output_margin=output_margin)
        assert bits(model.predict(mixed, output_margin=output_margin)[mine]) == bits(alone)
    assert len(np.unique(alone)) > 20
