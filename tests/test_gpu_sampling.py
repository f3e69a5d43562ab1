"""Row and column subsampling on the GPU ("Subsampling") against its NumPy restatement
(tests/forest_sampling_oracle.py): the single trainer, the batched trainer, cross_validate and train_model.  Every
round the oracle is handed the device's float32 probabilities (the device's expf may differ from NumPy's in the last
bits, as in test_gpu_trainer.py) and everything downstream -- the quantised gradients with their zeros, every tree, the
margins of ALL rows, the evaluation error -- is compared bit for bit."""
import numpy as np
import pytest

import forest_cv_oracle as cv_oracle
import forest_sampling_oracle as sampling
import forest_train_oracle as oracle
from forest_train_oracle import make_data

pytestmark = pytest.mark.gpu
MODEL_KEYS = ("feature", "threshold", "yes", "no", "missing", "tree_offsets")
FOUR = ["subsample", "colsample_bytree", "colsample_bylevel", "sample_seed"]


def heap_equal(device, expected):
    """A device heap (a batch's has the slots of its largest depth) against an oracle heap."""
    info, leaf = device
    slots = expected["state"].shape[0]
    assert not info[slots:, 0].any()
    info, leaf = info[:slots], leaf[:slots]
    assert np.array_equal(info[:, 0], expected["state"])
    split = expected["state"] == oracle.SPLIT
    assert np.array_equal(info[split, 1], expected["feature"][split])
    assert np.array_equal(info[split, 2], expected["bin"][split])
    assert np.array_equal(info[split, 3], expected["default_left"][split])
    leaves = expected["state"] == oracle.LEAF
    assert np.array_equal(leaf[leaves].view(np.uint32), expected["leaf"][leaves].view(np.uint32))


def same_model(a, b):
    return all(a.arrays[key].dtype == b.arrays[key].dtype and a.arrays[key].tobytes() == b.arrays[key].tobytes()
               for key in MODEL_KEYS) and a.arrays["base_margin"] == b.arrays["base_margin"]


def splits(trees):
    return sum(int(np.count_nonzero(tree["state"] == oracle.SPLIT)) for tree in trees)


def level_of(node):
    return int(node + 1).bit_length() - 1


def rows_through(tree, node_bins, rows=None):
    """int[slots]: how many of `rows` (bool mask, default all) pass through every node of the heap tree."""
    n = node_bins.shape[1]
    weight = np.ones(n, np.int64) if rows is None else np.asarray(rows).astype(np.int64)
    node = np.zeros(n, np.int64)
    counts = np.zeros(tree["state"].shape[0], np.int64)
    counts[0] = weight.sum()
    while True:
        moving = np.nonzero(tree["state"][node] == oracle.SPLIT)[0]      # a row at a leaf stays there
        if moving.size == 0:
            return counts
        at = node[moving]
        x = node_bins[tree["feature"][at], moving]
        left = np.where(x == oracle.MISSING, tree["default_left"][at] != 0, x < tree["bin"][at])
        node[moving] = np.where(left, 2 * at + 1, 2 * at + 2)
        np.add.at(counts, node[moving], weight[moving])


def check_single(trainer, booster, x, ex, ey, rounds):
    """Grow `rounds` trees on a begun ForestTrainer and compare every round with the oracle Booster."""
    for round_ in range(rounds):
        before = trainer.margins()
        error = trainer.step()
        p, gh = trainer.probabilities(), trainer.gradients()
        assert np.allclose(p, oracle.sigmoid32(before), rtol=3e-7, atol=0)       # written for EVERY row, drawn or not
        tree, expected_gh = booster.step(p)
        assert np.array_equal(gh, expected_gh), round_
        assert not gh[~booster.row_masks[-1]].any()
        heap_equal(trainer.last_heap, tree)
        margins = trainer.margins()
        assert np.array_equal(margins.view(np.uint32), booster.margins().view(np.uint32)), round_
        model = trainer.model()
        assert np.array_equal(margins.view(np.uint32), model.predict(x, output_margin=True).view(np.uint32)), round_
        if ex is not None:
            assert np.array_equal(trainer.eval_margins().view(np.uint32),
                                  model.predict(ex, output_margin=True).view(np.uint32)), round_
            assert error == oracle.custom_error(model.predict(ex), ey), round_


# ---- the single trainer -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def odd():
    """1003 rows (no multiple of 256 or 512) x 7 features with NaNs, and 301 evaluation rows."""
    x, y = make_data(1003, 7, 61)
    ex, ey = make_data(301, 7, 62)
    return x, y, ex, ey


SINGLE = [dict(subsample=0.5), dict(colsample_bytree=0.5), dict(colsample_bylevel=0.5),
          dict(subsample=0.5, colsample_bytree=0.5, colsample_bylevel=0.5, sample_seed=(1 << 63) - 1)]


@pytest.mark.parametrize("device_form", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("fractions", SINGLE, ids=["rows", "bytree", "bylevel", "all"])
def test_single_trainer_matches_the_oracle(odd, fractions, device_form):
    import doppel_speller_amd as ds
    from doppel_speller_amd import _lib
    x, y, ex, ey = odd
    parameters = dict(max_depth=3, eta=0.3, **fractions)
    trainer = ds.ForestTrainer()
    if device_form:
        d_x, d_ex = _lib.DeviceArray.from_host(x), _lib.DeviceArray.from_host(ex)
        trainer.begin_device(d_x, 1003, y, d_ex, 301, ey, **parameters)
        d_x.free()
        d_ex.free()
    else:
        trainer.begin(x, y, ex, ey, **parameters)
    booster = sampling.Booster(x, y, parameters)
    check_single(trainer, booster, x, ex, ey, 4)
    trainer.close()
    assert splits(booster.trees) >= 4
    if "subsample" in fractions:
        assert all(350 < drawn.sum() < 650 for drawn in booster.row_masks)          # 10 sigma of Binomial(1003, 0.5)
    else:
        assert all(drawn.all() for drawn in booster.row_masks)
    if "colsample_bytree" in fractions:                                            # k_tree = floor(0.5 * 7) = 3
        assert all(masks.any(axis=0).sum() <= 3 for masks in booster.masks)
    plain = sampling.Booster(x, y, dict(max_depth=3, eta=0.3))
    for _ in range(4):
        plain.step()
    assert not np.array_equal(plain.margins(), booster.margins())                  # the sampling changed the model


def test_defaults_and_fractions_of_one_grow_the_unsampled_trees(odd):
    import doppel_speller_amd as ds
    x, y, ex, ey = odd
    plain = ds.ForestTrainer().fit(x, y, num_boost_round=4, max_depth=3, eta=0.3)
    ones = ds.ForestTrainer().fit(x, y, num_boost_round=4, max_depth=3, eta=0.3, subsample=1, colsample_bytree=1.0,
                                  colsample_bylevel=1.0, sample_seed=99)
    assert same_model(plain, ones)
    seeded = ds.ForestTrainer().fit(x, y, num_boost_round=4, max_depth=3, eta=0.3, subsample=0.5, sample_seed=1)
    again = ds.ForestTrainer().fit(x, y, num_boost_round=4, max_depth=3, eta=0.3, subsample=0.5, sample_seed=1)
    other = ds.ForestTrainer().fit(x, y, num_boost_round=4, max_depth=3, eta=0.3, subsample=0.5, sample_seed=2)
    assert same_model(seeded, again) and not same_model(seeded, other) and not same_model(seeded, plain)


def test_one_tenth_subsample_on_near_empty_histograms():
    """300 rows, subsample 0.1, depth 5, min_child_weight 0: about 30 rows carry gradients, the deeper nodes hold a
    handful of them, most boundaries leave a side without a drawn row, and which child is built follows the counts of
    ALL rows, drawn or not."""
    import doppel_speller_amd as ds
    x, y = make_data(300, 7, 3)
    parameters = dict(max_depth=5, eta=0.5, min_child_weight=0.0, subsample=0.1)
    trainer = ds.ForestTrainer().begin(x, y, **parameters)
    booster = sampling.Booster(x, y, parameters)
    check_single(trainer, booster, x, None, None, 6)
    trainer.close()
    assert all(10 <= drawn.sum() <= 60 for drawn in booster.row_masks)
    deepest = max(level_of(node) for tree in booster.trees for node in np.nonzero(tree["state"] == oracle.SPLIT)[0])
    assert deepest >= 2
    fewest = min(int(rows_through(tree, booster.node_bins, drawn)[np.nonzero(tree["state"] != oracle.ABSENT)[0]].min())
                 for tree, drawn in zip(booster.trees, booster.row_masks))
    assert fewest <= 3                                      # a node was searched with next to no drawn row in it


def test_the_widest_feature_set_with_one_feature_per_tree():
    import doppel_speller_amd as ds
    x, y = make_data(600, 96, 7)
    parameters = dict(max_depth=3, eta=0.3, colsample_bytree=0.01, sample_seed=4)       # k_tree = max(1, 0) = 1
    trainer = ds.ForestTrainer().begin(x, y, **parameters)
    booster = sampling.Booster(x, y, parameters)
    check_single(trainer, booster, x, None, None, 3)
    trainer.close()
    used = []
    for tree, masks in zip(booster.trees, booster.masks):
        assert masks.any(axis=0).sum() == 1
        features = set(tree["feature"][tree["state"] == oracle.SPLIT].tolist())
        assert features <= {int(np.nonzero(masks[0])[0][0])}
        used.append(int(np.nonzero(masks[0])[0][0]))
    assert len(set(used)) > 1


# ---- excluded at level d, included at level d + 1: the parent - sibling subtraction of a feature that sat out ----------
def subtraction_events(booster):
    """(round, node, feature) of every split at a node whose histogram is parent - sibling (the sibling has no more rows
    than it, the left one wins a tie) on a feature that was outside the set of the parent's level."""
    events = []
    for round_, (tree, masks) in enumerate(zip(booster.trees, booster.masks)):
        counts = rows_through(tree, booster.node_bins)
        for node in np.nonzero(tree["state"] == oracle.SPLIT)[0]:
            if node == 0:
                continue
            left = node % 2 == 1
            sibling = node + 1 if left else node - 1
            built = counts[node] <= counts[sibling] if left else counts[node] < counts[sibling]
            feature, level = int(tree["feature"][node]), level_of(node)
            if not built and not masks[level - 1, feature] and masks[level, feature]:
                events.append((round_, int(node), feature))
    return events


def test_a_feature_that_sat_out_a_level_splits_a_subtracted_node(odd):
    import doppel_speller_amd as ds
    x, y, _, _ = odd
    base = dict(max_depth=3, eta=0.3, colsample_bylevel=0.5)
    seed = None
    for candidate in range(64):                             # chosen on the CPU, with NumPy's sigmoid
        trial = sampling.Booster(x, y, dict(base, sample_seed=candidate))
        for _ in range(3):
            trial.step()
        if subtraction_events(trial):
            seed = candidate
            break
    assert seed is not None
    parameters = dict(base, sample_seed=seed)
    trainer = ds.ForestTrainer().begin(x, y, **parameters)
    booster = sampling.Booster(x, y, parameters)
    check_single(trainer, booster, x, None, None, 3)        # every split equals the oracle's, that one included
    trainer.close()
    assert subtraction_events(booster), "the case did not happen with the device's probabilities"


# ---- the batched trainer ------------------------------------------------------------------------------------------------
SETS = [dict(max_depth=3, eta=0.3),
        dict(max_depth=4, eta=0.3, subsample=0.6),
        dict(max_depth=2, eta=0.3, subsample=0.7, colsample_bytree=0.5, colsample_bylevel=0.5, sample_seed=11)]
BATCH_ROUNDS = 4


def run_batch(x, y, fold, models, rounds):
    import doppel_speller_amd as ds
    batch = ds.ForestTrainerBatch().begin(x, y, fold, models)
    record = []
    for _ in range(rounds):
        errors = batch.step()
        record.append(dict(errors=errors, heaps=[(h[0].copy(), h[1].copy()) for h in batch.last_heap],
                           margins=[batch.margins(m) for m in range(len(models))],
                           probabilities=[batch.probabilities(m) for m in range(len(models))],
                           gradients=[batch.gradients(m) for m in range(len(models))]))
    return batch, record


@pytest.fixture(scope="module")
def batched():
    """5003 rows x 7 integer-valued features, 2 folds x 3 parameter sets in ONE batch.  Every feature has the same
    distinct values in each fold's training part as in the whole matrix, so ForestTrainer's own cuts of a training part
    are the batch's cuts."""
    import doppel_speller_amd as ds
    rng = np.random.RandomState(71)
    x = rng.randint(0, 20, (5003, 7)).astype(np.float32)
    y = (x[:, 0] + x[:, 1] - 0.5 * x[:, 2] + rng.randn(5003) * 3 > 12).astype(np.float32)
    fold = ds.fold_assignment(None, 2, seed=6, n=5003)
    models = [dict(one, held_out=k) for one in SETS for k in range(2)]
    batch, record = run_batch(x, y, fold, models, BATCH_ROUNDS)
    return x, y, fold, models, batch, record


def test_batch_models_match_the_oracle_every_round(batched):
    x, y, fold, models, batch, record = batched
    assert all(list(one) == list(cv_oracle.DEFAULTS) + FOUR for one in batch.parameters)
    per_feature = oracle.cuts(x)
    node_bins = oracle.bins(x, per_feature)
    counts = np.array([c.size for c in per_feature])
    assert np.array_equal(batch.bins(), node_bins)
    for m, model in enumerate(models):
        held = fold == model["held_out"]
        booster = sampling.Booster(x, y, model, fold, model["held_out"], per_feature)
        for round_, step in enumerate(record):
            p, gh = step["probabilities"][m], step["gradients"][m]
            tree, expected_gh = booster.step(p)
            assert np.array_equal(gh, expected_gh), (m, round_)
            assert not gh[held].any()
            heap_equal(step["heaps"][m], tree)
            if m < 2:       # the unsampled set: what the parent's code path gives, through the existing oracle
                plain = dict(cv_oracle.DEFAULTS, **model)
                assert np.array_equal(gh, cv_oracle.zeroed(oracle.gradients(p, y, 5.0), fold, model["held_out"]))
                heap_equal(step["heaps"][m], cv_oracle.grow(node_bins, counts, gh, fold, plain)[0])
            margins = step["margins"][m]
            assert np.array_equal(margins.view(np.uint32), booster.margins().view(np.uint32)), (m, round_)
            forest = batch.model(m, round_ + 1)
            assert step["errors"][m] == oracle.custom_error(forest.predict(x[held]), y[held]), (m, round_)
        assert splits(booster.trees) >= BATCH_ROUNDS
        if model.get("subsample", 1.0) < 1:
            drawn = booster.row_masks[0]
            assert 0.4 * (~held).sum() < drawn.sum() < 0.9 * (~held).sum() and not drawn[held].any()


def test_batch_models_equal_the_single_trainer_on_their_training_rows(batched):
    import doppel_speller_amd as ds
    x, y, fold, models, batch, record = batched
    for k in range(2):
        for f in range(7):
            assert np.array_equal(np.unique(x[fold != k, f]), np.unique(x[:, f]))
    for m, model in enumerate(models):
        train, held = fold != model["held_out"], fold == model["held_out"]
        parameters = {name: value for name, value in model.items() if name != "held_out"}
        single = ds.ForestTrainer().begin(x[train], y[train], x[held], y[held], **parameters)
        assert np.array_equal(single.cuts, batch.cuts) and np.array_equal(single.cut_offsets, batch.cut_offsets)
        slots = (2 << model["max_depth"]) - 1
        for round_, step in enumerate(record):
            single.step()
            info, leaf = single.last_heap
            assert info.tobytes() == step["heaps"][m][0][:slots].tobytes(), (m, round_)
            assert leaf.tobytes() == step["heaps"][m][1][:slots].tobytes(), (m, round_)
            assert single.gradients().tobytes() == step["gradients"][m][train].tobytes(), (m, round_)
        margins = record[-1]["margins"][m]
        assert margins[train].tobytes() == single.margins().tobytes()
        assert margins[held].tobytes() == single.eval_margins().tobytes()
        assert single.history == batch.history[m]
        single.close()


def test_a_capped_grid_changes_no_byte(batched):
    from doppel_speller_amd import tuning
    x, y, fold, models, _, record = batched
    tuning.batch_option("max_blocks", 3)
    try:
        batch, capped = run_batch(x, y, fold, models, BATCH_ROUNDS)
        batch.close()
    finally:
        tuning.batch_option("max_blocks", 0)
    for step, other in zip(record, capped):
        assert step["errors"] == other["errors"]
        for name in ("margins", "probabilities", "gradients"):
            assert all(a.tobytes() == b.tobytes() for a, b in zip(step[name], other[name])), name
        assert all(a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
                   for a, b in zip(step["heaps"], other["heaps"]))


def test_an_inactive_round_does_not_advance_the_models_streams(odd):
    """Model 1 sits out the batch's third step: its third tree comes with the fourth step and is the oracle's tree of
    ITS round 2."""
    import doppel_speller_amd as ds
    x, y, _, _ = odd
    fold = ds.fold_assignment(None, 2, seed=2, n=1003)
    models = [dict(max_depth=3, eta=0.3, subsample=0.5, colsample_bytree=0.5, sample_seed=1, held_out=0),
              dict(max_depth=3, eta=0.3, subsample=0.5, colsample_bylevel=0.5, sample_seed=2, held_out=1)]
    batch = ds.ForestTrainerBatch().begin(x, y, fold, models)
    per_feature = oracle.cuts(x)
    boosters = [sampling.Booster(x, y, model, fold, model["held_out"], per_feature) for model in models]
    for active in ([1, 1], [1, 1], [1, 0], [1, 1]):
        errors = batch.step(active)
        for m in np.nonzero(active)[0]:
            tree, expected_gh = boosters[m].step(batch.probabilities(m))
            assert np.array_equal(batch.gradients(m), expected_gh)
            heap_equal(batch.last_heap[m], tree)
            assert np.array_equal(batch.margins(m).view(np.uint32), boosters[m].margins().view(np.uint32))
        assert (errors[1] is None) == (active[1] == 0)
    assert [len(trees) for trees in batch.trees] == [4, 3] == [len(booster.trees) for booster in boosters]
    trains = fold != 1                                      # model 1's third tree drew the rows of t = 2, not of t = 3
    drawn = batch.gradients(1).any(axis=1)[trains]
    n_train = int(trains.sum())
    undrawn_by_chance = ~sampling.row_mask(2, 2, n_train, 0.5)
    assert not drawn[undrawn_by_chance].any()
    assert drawn[~sampling.row_mask(2, 3, n_train, 0.5)].any()
    batch.close()


# ---- cross_validate -----------------------------------------------------------------------------------------------------
def test_cross_validate_with_sampling_on_a_small_grid():
    import doppel_speller_amd as ds
    x, y = make_data(3000, 7, 81)
    grid = ds.parameter_grid(subsample=[0.5, 1.0], colsample_bytree=[0.5, 1.0])
    assert len(grid) == 4
    call = dict(n_folds=3, seed=5, num_boost_round=10, early_stopping_rounds=10)
    cv = ds.cross_validate(x, y, grid, **call)
    again = ds.cross_validate(x, y, grid, models_per_batch=3, **call)
    assert cv.results.equals(again.results) and cv.history == again.history and cv.fold_history == again.fold_history
    assert cv.best_parameters == again.best_parameters and same_model(cv.model, again.model)
    assert list(cv.results.columns) == list(cv_oracle.DEFAULTS) + FOUR + ["best_iteration", "error", "rounds",
                                                                          "fold_errors"]
    assert cv.results["subsample"].tolist() == [0.5, 0.5, 1.0, 1.0]
    assert cv.results["colsample_bytree"].tolist() == [0.5, 1.0, 0.5, 1.0]
    assert (cv.results["rounds"] == 10).all() and list(cv.best_parameters) == list(cv_oracle.DEFAULTS) + FOUR
    model = ds.ForestTrainer().fit(x, y, num_boost_round=cv.best_iteration + 1, **cv.best_parameters)
    assert model.n_trees == cv.model.n_trees == cv.best_iteration + 1 and same_model(cv.model, model)
    # the out-of-fold curves: the same models stepped in one batch, every round checked against the oracle
    models = [dict(one, held_out=k) for one in grid for k in range(3)]
    batch = ds.ForestTrainerBatch().begin(x, y, cv.folds, models)
    per_feature = oracle.cuts(x)
    boosters = [sampling.Booster(x, y, model, cv.folds, model["held_out"], per_feature) for model in models]
    curves = [[] for _ in models]
    for round_ in range(10):
        errors = batch.step()
        for m, model in enumerate(models):
            tree, expected_gh = boosters[m].step(batch.probabilities(m))
            assert np.array_equal(batch.gradients(m), expected_gh), (m, round_)
            heap_equal(batch.last_heap[m], tree)
            margins = batch.margins(m)
            assert np.array_equal(margins.view(np.uint32), boosters[m].margins().view(np.uint32)), (m, round_)
            held = cv.folds == model["held_out"]
            expected = oracle.custom_error(batch.model(m).predict(x[held]), y[held])
            assert errors[m] == expected
            curves[m].append(expected)
    batch.close()
    assert cv.fold_history == [[curves[p * 3 + k] for k in range(3)] for p in range(4)]
    assert cv.history == [[sum(curves[p * 3 + k][r] for k in range(3)) for r in range(10)] for p in range(4)]
    assert len({boosters[p * 3].margins().tobytes() for p in range(4)}) == 4   # the four sets trained differently


# ---- train_model --------------------------------------------------------------------------------------------------------
def test_train_model_with_sampling_equals_fit_on_the_host_sets():
    import doppel_speller_amd as ds
    from doppel_speller_amd import synth
    w = synth.make_workload(2000, 400, seed=21, query_seed=22)
    truth, train = synth._to_strings(w.t_flat, w.t_off), synth._to_strings(w.q_flat, w.q_off)
    ids = np.where(w.actual_row >= 0, w.title_id[np.maximum(w.actual_row, 0)], -1)
    data = dict(top_n=10, sample_n=5, seed=9, transform=False)
    fit = dict(num_boost_round=12, early_stopping_rounds=12)
    sampled = dict(subsample=0.7, colsample_bytree=0.7, sample_seed=3)
    result = ds.train_model(truth, w.title_id, train, ids, **data, **fit, **sampled)
    fe = ds.FeatureEngineering(truth, w.title_id, train, ids, **data)
    sets = fe.generate_train_and_evaluation_data_sets()
    trainer = ds.ForestTrainer()
    model = trainer.fit(*sets, **fit, **sampled)
    assert same_model(result.model, model) and result.history == trainer.history
    assert result.best_iteration == trainer.best_iteration and result.model.n_trees >= 1
    plain = ds.train_model(truth, w.title_id, train, ids, **data, **fit)
    assert not same_model(result.model, plain.model)
    used = set(result.model.arrays["feature"][result.model.arrays["feature"] >= 0].tolist())
    assert len(used) > 1
