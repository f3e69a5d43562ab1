"""Continuing from a model on the GPU ("Continuing from a model"): k rounds followed by m rounds
seeded with those k trees are the k + m rounds of a straight run, bit for bit; the seed kernel against the NumPy tree
walk of tests/forest_continue_oracle.py; new data, early stopping, the batched trainer and the refusals.  Where a round
is compared with the oracle, the oracle is handed the device's float32 probabilities (as in test_gpu_sampling.py) and
everything downstream is compared bit for bit."""
import ctypes

import numpy as np
import pytest

import forest_continue_oracle as continued
import forest_train_oracle as oracle
from forest_train_oracle import make_data
from test_continue_cpu import (BASE, BASE_PARAMETERS, K, M, SAMPLED, STOPPING, STOPPING_PARAMETERS, base_data,
                               between_cuts_forest)
from test_gpu_sampling import heap_equal, same_model

pytestmark = pytest.mark.gpu


def bits(a):
    return np.asarray(a).tobytes()


def no_stop(rounds):
    return dict(num_boost_round=rounds, early_stopping_rounds=rounds)


# ---- 1. the identity ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def base():
    return base_data()


@pytest.mark.parametrize("device_form", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("extra", [{}, SAMPLED], ids=["plain", "sampled"])
def test_k_plus_m_rounds_equal_k_rounds_continued_for_m(base, extra, device_form):
    import doppel_speller_amd as ds
    from doppel_speller_amd import _lib
    x, y, ex, ey = base
    parameters = dict(BASE_PARAMETERS, **extra)
    arrays = []

    def fit(trainer, rounds, **more):
        if not device_form:
            return trainer.fit(x, y, ex, ey, **no_stop(rounds), **parameters, **more)
        d_x, d_ex = _lib.DeviceArray.from_host(x), _lib.DeviceArray.from_host(ex)
        arrays.extend([d_x, d_ex])
        return trainer.fit_device(d_x, x.shape[0], y, d_ex, ex.shape[0], ey, **no_stop(rounds), **parameters, **more)

    straight, first, second = ds.ForestTrainer(), ds.ForestTrainer(), ds.ForestTrainer()
    fit(straight, K + M)
    fit(first, K)
    init = first.model()
    assert init.n_trees == K and same_model(init, straight.model(K)) and same_model(init, straight.model().head(K))
    returned = fit(second, M, init_model=init)
    assert len(second.trees) == M and same_model(second.model(), straight.model())
    for n in range(M + 1):
        assert same_model(second.model(n), straight.model(K + n))
    assert bits(second.margins()) == bits(straight.margins())
    assert bits(second.eval_margins()) == bits(straight.eval_margins())
    assert second.history == straight.history[K:] and second.initial_error == straight.history[K - 1]
    assert first.initial_error is None and straight.initial_error is None
    best = int(np.argmin(second.history))
    assert second.best_iteration == K + best and returned.n_trees == K + best + 1
    assert same_model(returned, straight.model(K + best + 1))
    if extra:                       # the draws do shape the new trees: another seed, other trees
        again = ds.ForestTrainer()
        again.fit(x, y, ex, ey, **no_stop(M), **dict(parameters, sample_seed=SAMPLED["sample_seed"] + 1), init_model=init)
        assert not same_model(again.model(), second.model())
        again.close()
    for trainer in (straight, first, second):
        trainer.close()
    for array in arrays:
        array.free()


def test_step_form_and_metrics_read_the_seeded_margins(base):
    """begin(init_model=) + step(): the metrics of the first new round are those of the straight run's round k."""
    import doppel_speller_amd as ds
    x, y, ex, ey = base
    straight = ds.ForestTrainer().begin(x, y, ex, ey, eval_metrics=("auc", "logloss"), **BASE_PARAMETERS)
    for _ in range(K + 2):
        straight.step()
    second = ds.ForestTrainer().begin(x, y, ex, ey, eval_metrics=("auc", "logloss"), **BASE_PARAMETERS,
                                      init_model=straight.model(K))
    assert second.initial_error == straight.history[K - 1] and second.history == []
    assert bits(second.margins()) == bits(straight.model(K).predict(x, output_margin=True))
    for _ in range(2):
        second.step()
    assert second.metric_counts == straight.metric_counts[K:]
    assert second.history == straight.history[K:]
    straight.close()
    second.close()


def test_train_model_continues_from_the_head_of_a_straight_run():
    import doppel_speller_amd as ds
    from doppel_speller_amd import synth
    w = synth.make_workload(2000, 400, seed=21, query_seed=22)
    truth, train = synth._to_strings(w.t_flat, w.t_off), synth._to_strings(w.q_flat, w.q_off)
    ids = np.where(w.actual_row >= 0, w.title_id[np.maximum(w.actual_row, 0)], -1)
    data = dict(top_n=10, sample_n=5, seed=9, transform=False)
    sampled = dict(subsample=0.7, colsample_bytree=0.7, sample_seed=3, eta=0.3)
    fe = ds.FeatureEngineering(truth, w.title_id, train, ids, **data)
    sets = fe.generate_train_and_evaluation_data_sets()
    trainer = ds.ForestTrainer()
    trainer.fit(*sets, **no_stop(K + M), **sampled)
    whole = trainer.model()
    assert whole.n_trees == K + M
    init = whole.head(K)
    result = ds.train_model(truth, w.title_id, train, ids, **data, **no_stop(M), **sampled, init_model=init, cover=True)
    assert result.history == trainer.history[K:] and result.initial_error == trainer.history[K - 1]
    best = int(np.argmin(result.history))
    assert result.best_iteration == K + best and result.model.n_trees == K + best + 1
    assert same_model(result.model, whole.head(K + best + 1))
    assert bits(result.feature_importance) == bits(result.model.feature_importance())
    assert result.model.cover is not None and result.model.cover.shape == (result.model.n_nodes,)   # the WHOLE forest's
    plain = ds.train_model(truth, w.title_id, train, ids, **data, **no_stop(M), **sampled)
    assert plain.initial_error is None and same_model(plain.model, whole.head(plain.model.n_trees))
    trainer.close()


# ---- 2. the seed kernel against the NumPy walk ---------------------------------------------------------------------------
def check_seed(x, y, ex, ey, trees, **parameters):
    """begin(init_model=from_trees(trees)): margins, evaluation margins and initial error before any step."""
    import doppel_speller_amd as ds
    init = ds.ForestModel.from_trees(trees, x.shape[1])
    arrays = continued.flat_forest(trees)
    trainer = ds.ForestTrainer().begin(x, y, ex, ey, init_model=init, **parameters)
    expected, expected_eval = continued.leaf_sums(arrays, x), continued.leaf_sums(arrays, ex)
    assert bits(trainer.margins()) == bits(np.float32(0.0) + expected)
    assert bits(trainer.eval_margins()) == bits(np.float32(0.0) + expected_eval)
    assert bits(init.predict(ex, output_margin=True)) == bits(np.float32(0.0) + expected_eval)
    assert trainer.initial_error == oracle.custom_error(init.predict(ex), ey)
    return trainer, init, arrays


def wide_data(n, nf, seed):
    x, y = make_data(n, nf, seed)
    x[::7, 0] = np.nan                          # NaN and -0.0 in a column of every width
    x[1::7, 0] = np.float32(-0.0)
    return x, y


@pytest.mark.parametrize("nf", [1, 47, 48, 96])
def test_seed_at_the_staging_layouts(nf):
    """47 (an odd row stride as it is), 48 (padded by one) and 96 features (the largest LDS image), and one feature;
    600 rows: two full workgroups and a part of one."""
    x, y = wide_data(600, nf, 30 + nf)
    ex, ey = wide_data(333, nf, 130 + nf)
    trees = continued.random_forest(7, 5, nf, nf)
    trainer, _, arrays = check_seed(x, y, ex, ey, trees, max_depth=3)
    events = {}
    continued.leaf_sums(arrays, x, events)
    assert events["nan"] > 50 and events["yes"] > 500 and events["no"] > 500
    assert len(np.unique(trainer.margins())) > 10
    trainer.close()


@pytest.mark.parametrize("n", [1, 257])
def test_seed_of_one_row_and_of_one_row_more_than_a_workgroup(n):
    x, y = wide_data(n, 7, 40 + n)
    ex, ey = wide_data(n, 7, 50 + n)
    check_seed(x, y, ex, ey, continued.random_forest(5, 4, 7, n), max_depth=2)[0].close()


def test_seed_with_one_workgroup_strides_over_all_rows(base):
    from doppel_speller_amd import tuning
    x, y, ex, ey = base
    trees = between_cuts_forest(x)
    plain = check_seed(x, y, ex, ey, trees, **BASE_PARAMETERS)[0]
    tuning.batch_option("max_blocks", 1)
    try:
        capped = check_seed(x, y, ex, ey, trees, **BASE_PARAMETERS)[0]
    finally:
        tuning.batch_option("max_blocks", 0)
    assert bits(capped.margins()) == bits(plain.margins()) and capped.initial_error == plain.initial_error
    plain.close()
    capped.close()


def test_a_host_matrix_larger_than_one_upload_chunk_is_seeded_in_two():
    """A host matrix is uploaded in chunks of at most 64 MiB: 174,762 rows of 96 features.  180,001 rows take a second
    chunk, whose leaf sums land behind the first one's."""
    import doppel_speller_amd as ds
    n, nf = 180001, 96
    assert (64 << 20) // (4 * nf) < n - 256
    rng = np.random.RandomState(8)
    x = rng.randn(n, nf).astype(np.float32)
    x[::5, 3] = np.nan
    y = (x[:, 0] > 0.5).astype(np.float32)
    trees = continued.random_forest(3, 4, nf, 8)
    arrays = continued.flat_forest(trees)
    init = ds.ForestModel.from_trees(trees, nf)
    trainer = ds.ForestTrainer().begin(x, y, init_model=init, max_depth=2, max_bin=16)
    expected = np.float32(0.0) + continued.leaf_sums(arrays, x)
    margins = trainer.margins()
    assert bits(margins) == bits(expected) and len(np.unique(expected[174762:])) > 10
    assert trainer.initial_error is None
    trainer.close()


def tree_depth(tree):
    """Splits on the longest root-to-leaf path of one tree's arrays."""
    depth = np.zeros(tree["feature"].shape[0], np.int64)
    for i in range(tree["feature"].shape[0]):           # children come after their parent
        if tree["feature"][i] >= 0:
            depth[tree["yes"][i]] = depth[tree["no"][i]] = depth[i] + 1
    return int(depth.max())


def continue_against_the_oracle(trainer, booster, x, ex, ey, rounds, eval_sum):
    """`rounds` steps of a seeded trainer against a ContinueBooster fed the device's probabilities."""
    eval_bins = oracle.bins(ex, booster.per_feature)
    for round_ in range(rounds):
        error = trainer.step()
        tree, expected_gh = booster.step(trainer.probabilities())
        assert np.array_equal(trainer.gradients(), expected_gh), round_
        heap_equal(trainer.last_heap, tree)
        assert bits(trainer.margins()) == bits(booster.margins()), round_
        eval_sum = (eval_sum + tree["leaf"][oracle.route(tree, eval_bins)]).astype(np.float32)
        assert bits(trainer.eval_margins()) == bits(np.float32(0.0) + eval_sum), round_
        model = trainer.model()
        assert bits(model.predict(x, output_margin=True)) == bits(trainer.margins()), round_
        assert error == oracle.custom_error(model.predict(ex), ey), round_


def test_a_hand_built_model_between_the_cuts_is_continued_like_the_oracle(base):
    x, y, ex, ey = base
    trees = between_cuts_forest(x)
    parameters = dict(BASE_PARAMETERS, **SAMPLED)
    trainer, init, arrays = check_seed(x, y, ex, ey, trees, **parameters)
    booster = continued.ContinueBooster(x, y, arrays, parameters)
    continue_against_the_oracle(trainer, booster, x, ex, ey, 3, continued.leaf_sums(arrays, ex))
    assert trainer.model().n_trees == len(trees) + 3 and same_model(trainer.model(0), init)
    trainer.close()


def test_a_model_of_depth_eight_is_continued_at_depth_three(base):
    import doppel_speller_amd as ds
    x, y, ex, ey = base
    deep = ds.ForestTrainer()
    deep.fit(x, y, **no_stop(3), max_depth=8, eta=0.3, min_child_weight=0.0)
    init = deep.model()
    arrays = {key: init.arrays[key] for key in init.arrays}
    assert max(tree_depth(tree) for tree in ds.ForestModel.tree_list(arrays)) == 8
    trainer = ds.ForestTrainer().begin(x, y, ex, ey, init_model=init, max_depth=3, eta=0.3)
    assert bits(trainer.margins()) == bits(np.float32(0.0) + continued.leaf_sums(arrays, x)) == bits(deep.margins())
    booster = continued.ContinueBooster(x, y, arrays, dict(max_depth=3, eta=0.3))
    continue_against_the_oracle(trainer, booster, x, ex, ey, 2, continued.leaf_sums(arrays, ex))
    deep.close()
    trainer.close()


def test_a_model_of_zero_trees_is_a_fresh_fit(base):
    import doppel_speller_amd as ds
    x, y, ex, ey = base
    fresh = ds.ForestTrainer()
    fresh_model = fresh.fit(x, y, ex, ey, **no_stop(M), **BASE_PARAMETERS, **SAMPLED)
    empty = ds.ForestModel.from_trees([], 7)
    assert empty.n_trees == 0 and same_model(empty, fresh.model().head(0))
    seeded = ds.ForestTrainer()
    seeded_model = seeded.fit(x, y, ex, ey, **no_stop(M), **BASE_PARAMETERS, **SAMPLED, init_model=empty)
    assert same_model(seeded_model, fresh_model) and same_model(seeded.model(), fresh.model())
    assert seeded.history == fresh.history and seeded.best_iteration == fresh.best_iteration
    assert bits(seeded.margins()) == bits(fresh.margins()) and bits(seeded.eval_margins()) == bits(fresh.eval_margins())
    assert seeded.initial_error == continued.error_of(np.zeros(ex.shape[0], np.float32), ey) == int(ey.sum())
    fresh.close()
    seeded.close()


# ---- 3. new data ----------------------------------------------------------------------------------------------------------
def test_a_model_trained_on_one_matrix_is_continued_on_another(base):
    import doppel_speller_amd as ds
    x, y, ex, ey = base
    other, other_y = make_data(BASE["n"], BASE["nf"], BASE["other_seed"])
    first = ds.ForestTrainer()
    first.fit(x, y, **no_stop(K), **BASE_PARAMETERS)
    init = first.model()
    arrays = {key: init.arrays[key] for key in init.arrays}
    cuts_b = oracle.cuts(other)
    outside = [t for f, t in zip(arrays["feature"], arrays["threshold"]) if f >= 0 and t not in cuts_b[f]]
    assert len(outside) >= 10                  # thresholds that the bins of the new matrix cannot express
    trainer = ds.ForestTrainer().begin(other, other_y, ex, ey, init_model=init, **BASE_PARAMETERS)
    assert bits(trainer.margins()) == bits(np.float32(0.0) + continued.leaf_sums(arrays, other))
    assert bits(trainer.margins()) != bits(first.margins())
    booster = continued.ContinueBooster(other, other_y, arrays, BASE_PARAMETERS)
    continue_against_the_oracle(trainer, booster, other, ex, ey, M, continued.leaf_sums(arrays, ex))
    model = trainer.model()
    assert model.n_trees == K + M and same_model(model.head(K), init)
    assert bits(model.predict(other, output_margin=True)) == bits(trainer.margins())
    first.close()
    trainer.close()


# ---- 4. early stopping ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(STOPPING))
def test_early_stopping_looks_at_the_new_rounds_only(case):
    import doppel_speller_amd as ds
    seed, eval_seed, patience = STOPPING[case]
    x, y = make_data(BASE["n"], BASE["nf"], seed)
    ex, ey = make_data(BASE["n_eval"], BASE["nf"], eval_seed)
    first = ds.ForestTrainer()
    first.fit(x, y, ex, ey, **no_stop(K), **STOPPING_PARAMETERS)
    init = first.model()
    trainer = ds.ForestTrainer()
    model = trainer.fit(x, y, ex, ey, num_boost_round=K + 10, early_stopping_rounds=patience, init_model=init,
                        **STOPPING_PARAMETERS)
    history = trainer.history
    best = int(np.argmin(history))             # np.argmin: the first minimum
    assert best < len(history) - 1 < K + 10 - 1 and len(history) - 1 - best == patience     # it did stop early
    assert trainer.best_iteration == K + best and model.n_trees == trainer.best_iteration + 1
    assert same_model(model, trainer.model(best + 1)) and same_model(model.head(K), init)
    assert trainer.initial_error == first.history[-1] == oracle.custom_error(init.predict(ex), ey)
    if case == "initial_is_lower":             # as a candidate the init model would have won: it is none
        assert trainer.initial_error < min(history) and model.n_trees == K + 1
    else:
        assert best >= 1
    first.close()
    trainer.close()


# ---- 5. the batched trainer ------------------------------------------------------------------------------------------------
FOLDS = 3
SETS = [dict(max_depth=3, eta=0.3), dict(max_depth=4, eta=0.3, subsample=0.5, sample_seed=11)]


@pytest.fixture(scope="module")
def batched():
    """5003 rows x 7 integer-valued features, 3 folds x 2 parameter sets in ONE batch, every model started from a model
    of 5 trees grown on OTHER rows.  Every feature has the same distinct values in each fold's training part as in the
    whole matrix, so ForestTrainer's own cuts of a training part are the batch's cuts."""
    import doppel_speller_amd as ds
    rng = np.random.RandomState(73)
    x = rng.randint(0, 20, (5003, 7)).astype(np.float32)
    x[rng.rand(5003) < 0.1, 2] = np.nan
    y = (x[:, 0] + x[:, 1] - 0.5 * np.nan_to_num(x[:, 2]) + rng.randn(5003) * 3 > 12).astype(np.float32)
    before = rng.randint(0, 20, (1500, 7)).astype(np.float32) + np.float32(0.5)      # thresholds between x's cuts
    before_y = (before[:, 0] + before[:, 1] + rng.randn(1500) * 3 > 14).astype(np.float32)
    first = ds.ForestTrainer()
    first.fit(before, before_y, **no_stop(K), max_depth=3, eta=0.5)
    init = first.model()
    first.close()
    fold = ds.fold_assignment(None, FOLDS, seed=6, n=5003)
    models = [dict(one, held_out=k) for one in SETS for k in range(FOLDS)]
    batch = ds.ForestTrainerBatch().begin(x, y, fold, models, init_model=init)
    seeded = [batch.margins(m) for m in range(len(models))]
    record = []
    for _ in range(3):
        errors = batch.step()
        record.append(dict(errors=errors, heaps=[(h[0].copy(), h[1].copy()) for h in batch.last_heap],
                           margins=[batch.margins(m) for m in range(len(models))]))
    return x, y, fold, models, init, batch, seeded, record


def test_batch_is_seeded_once_per_row_for_every_model(batched):
    x, y, fold, models, init, batch, seeded, record = batched
    arrays = {key: init.arrays[key] for key in init.arrays}
    expected = np.float32(0.0) + continued.leaf_sums(arrays, x)
    assert len(np.unique(expected)) > 5
    assert all(bits(one) == bits(expected) for one in seeded)              # held-out rows included
    p = init.predict(x)
    for m, model in enumerate(models):
        held = fold == model["held_out"]
        assert batch.initial_errors[m] == oracle.custom_error(p[held], y[held])
    assert sum(batch.initial_errors[:FOLDS]) == sum(batch.initial_errors[FOLDS:]) == oracle.custom_error(p, y)
    assert same_model(batch.model(0, 0), init) and batch.model(0).n_trees == K + 3


def test_batch_models_equal_the_seeded_single_trainer_on_their_training_rows(batched):
    import doppel_speller_amd as ds
    x, y, fold, models, init, batch, seeded, record = batched
    for k in range(FOLDS):
        for f in range(7):
            values = x[:, f][~np.isnan(x[:, f])]
            part = x[fold != k, f]
            assert np.array_equal(np.unique(part[~np.isnan(part)]), np.unique(values))
    for m, model in enumerate(models):
        train, held = fold != model["held_out"], fold == model["held_out"]
        parameters = {name: value for name, value in model.items() if name != "held_out"}
        single = ds.ForestTrainer().begin(x[train], y[train], x[held], y[held], init_model=init, **parameters)
        assert np.array_equal(single.cuts, batch.cuts) and np.array_equal(single.cut_offsets, batch.cut_offsets)
        assert single.initial_error == batch.initial_errors[m]
        slots = (2 << model["max_depth"]) - 1
        for round_, step in enumerate(record):
            single.step()
            info, leaf = single.last_heap
            assert bits(info) == bits(step["heaps"][m][0][:slots]), (m, round_)
            assert bits(leaf) == bits(step["heaps"][m][1][:slots]), (m, round_)
        margins = record[-1]["margins"][m]
        assert bits(margins[train]) == bits(single.margins()) and bits(margins[held]) == bits(single.eval_margins())
        assert single.history == batch.history[m]
        assert same_model(single.model(), batch.model(m))
        single.close()


def test_cross_validate_continues_every_fold_and_refits_like_fit(batched):
    import doppel_speller_amd as ds
    x, y, _, _, init, _, _, _ = batched
    call = dict(n_folds=FOLDS, seed=5, num_boost_round=6, early_stopping_rounds=6)
    cv = ds.cross_validate(x, y, SETS, init_model=init, **call)
    p = init.predict(x)
    pooled = sum(oracle.custom_error(p[cv.folds == k], y[cv.folds == k]) for k in range(FOLDS))
    assert cv.initial_errors == [pooled, pooled] == cv.results["initial_error"].tolist()
    assert [len(curve) for curve in cv.history] == [6, 6] and (cv.results["rounds"] == 6).all()
    assert cv.best_iteration == cv.results["best_iteration"][cv.chosen] < 6          # the new rounds are counted
    trainer = ds.ForestTrainer()
    model = trainer.fit(x, y, num_boost_round=cv.best_iteration + 1, init_model=init, **cv.best_parameters)
    assert cv.model.n_trees == K + cv.best_iteration + 1 and same_model(cv.model, model)
    assert same_model(cv.model.head(K), init)
    trainer.close()
    # the curves: the same folds stepped in one batch
    models = [dict(one, held_out=k) for one in cv.parameters for k in range(FOLDS)]
    batch = ds.ForestTrainerBatch().begin(x, y, cv.folds, models, init_model=init)
    for _ in range(6):
        batch.step()
    assert cv.fold_history == [[batch.history[p_ * FOLDS + k] for k in range(FOLDS)] for p_ in range(2)]
    batch.close()
    plain = ds.cross_validate(x, y, SETS, refit=False, **call)
    assert not hasattr(plain, "initial_errors") and "initial_error" not in plain.results.columns
    assert plain.history != cv.history


# ---- 6. misuse --------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_trainer_as_it_was(base):
    import doppel_speller_amd as ds
    from doppel_speller_amd import _lib
    x, y, ex, ey = base
    library = _lib.lib()
    p = _lib.pointer
    error = ctypes.c_int64(-7)
    init = ds.ForestModel.from_trees(continued.random_forest(3, 3, 7, 1), 7)
    shifted = ds.ForestModel.from_trees(continued.random_forest(3, 3, 7, 1), 7, base_margin=0.25)
    narrow = ds.ForestModel.from_trees(continued.random_forest(3, 3, 6, 1), 6)

    def refused(handle, model, features, eval_features, text):
        status = library.ds_trainer_seed(handle, model.handle if model else None, p(features), p(eval_features),
                                         ctypes.byref(error))
        assert status == -1 and text in library.ds_last_error().decode() and error.value == -7, text

    trainer = ds.ForestTrainer().begin(x, y, ex, ey, **BASE_PARAMETERS)
    refused(trainer.handle, None, x, ex, "forest is null")
    refused(trainer.handle, narrow, x, ex, "the forest has 6 features, the trainer 7")
    refused(trainer.handle, shifted, x, ex, "base margin")
    refused(trainer.handle, init, None, ex, "features is null")
    refused(trainer.handle, init, x, None, "eval_features goes with")
    assert not trainer.margins().any() and not trainer.eval_margins().any()      # nothing was written
    assert library.ds_trainer_seed(trainer.handle, init.handle, p(x), p(ex), ctypes.byref(error)) == 0
    assert error.value == oracle.custom_error(init.predict(ex), ey)
    seeded = trainer.margins()
    error.value = -7
    refused(trainer.handle, init, x, ex, "already seeded")
    assert library.ds_trainer_set_eval(trainer.handle, p(ex), p(ey), ex.shape[0]) == -1
    assert "before the trainer is seeded" in library.ds_last_error().decode()
    assert bits(trainer.margins()) == bits(seeded)
    trainer.step()
    trainer.close()

    stepped = ds.ForestTrainer().begin(x, y, **BASE_PARAMETERS)
    refused(stepped.handle, init, x, ex, "eval_features goes with")              # the trainer has no evaluation set
    stepped.step()
    after = stepped.margins()
    refused(stepped.handle, init, x, None, "before the first round")
    assert bits(stepped.margins()) == bits(after)
    assert stepped.step() is None                                                # and it goes on as before
    stepped.close()

    for model, text in ((narrow, "6 features"), (shifted, "base margin"), ("a path", "must be a ForestModel")):
        with pytest.raises(ValueError, match=text):
            ds.ForestTrainer().fit(x, y, init_model=model)

    fold = (np.arange(x.shape[0]) % 2).astype(np.uint8)
    batch = ds.ForestTrainerBatch().begin(x, y, fold, [dict(BASE_PARAMETERS, held_out=0), dict(BASE_PARAMETERS)])
    errors = np.full(2, -7, np.int64)
    for model, text in ((narrow, "6 features"), (shifted, "base margin")):
        assert library.ds_trainer_batch_seed(batch.handle, model.handle, p(x), p(errors)) == -1
        assert text in library.ds_last_error().decode()
    assert library.ds_trainer_batch_seed(batch.handle, init.handle, p(x), p(errors)) == 0
    held = fold == 0
    assert errors.tolist() == [oracle.custom_error(init.predict(x[held]), y[held]), -1]
    assert library.ds_trainer_batch_seed(batch.handle, init.handle, p(x), p(errors)) == -1
    assert "already seeded" in library.ds_last_error().decode()
    batch.step()
    assert library.ds_trainer_batch_seed(batch.handle, init.handle, p(x), p(errors)) == -1
    assert "before the first step" in library.ds_last_error().decode()
    assert batch.step() is not None
    batch.close()
