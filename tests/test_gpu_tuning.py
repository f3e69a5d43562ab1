"""cross_validate and tune_model_parameters on the GPU: independence of the batch size, determinism, the stepping rule
replayed on the host from a batch stepped past the stop, the refit model against ForestTrainer.fit, and the one-call
form from raw titles against cross_validate on the host copy of the same sets.  Everything bit for bit."""
import numpy as np
import pytest

from forest_train_oracle import make_data

pytestmark = pytest.mark.gpu
MODEL_KEYS = ("feature", "threshold", "yes", "no", "missing", "tree_offsets")
# the parameter sets of test_gpu_trainer_batch.py's mixed batch
GRID = [dict(max_depth=5), dict(max_depth=2, eta=0.3, min_child_weight=0.0),
        dict(max_depth=2, eta=0.3, min_child_weight=0.5, reg_lambda=0.0), dict(max_depth=4, min_child_weight=2.0, beta=1.0)]


def same_model(a, b):
    return all(a.arrays[key].dtype == b.arrays[key].dtype and a.arrays[key].tobytes() == b.arrays[key].tobytes()
               for key in MODEL_KEYS) and a.arrays["base_margin"] == b.arrays["base_margin"]


def same_result(a, b):
    return a.results.equals(b.results) and a.history == b.history and a.fold_history == b.fold_history and \
        a.best_parameters == b.best_parameters and a.best_iteration == b.best_iteration and a.chosen == b.chosen and \
        a.folds.tobytes() == b.folds.tobytes() and same_model(a.model, b.model)


# ---- 4. batch independence and determinism ------------------------------------------------------------------------------
def test_the_result_does_not_depend_on_the_batches_and_repeats_byte_for_byte():
    import doppel_speller_amd as ds
    x, y = make_data(5003, 17, 41)
    call = dict(n_folds=2, seed=4, num_boost_round=12, early_stopping_rounds=4)
    first = ds.cross_validate(x, y, GRID, models_per_batch=2, **call)          # K: one set per batch
    assert np.array_equal(first.folds, ds.fold_assignment(None, 2, seed=4, n=5003))
    assert list(first.results.columns) == ["max_depth", "eta", "min_child_weight", "reg_lambda", "beta",
                                           "best_iteration", "error", "rounds", "fold_errors"]
    assert len(first.results) == 4 and first.model.n_trees == first.best_iteration + 1
    for p in range(4):
        assert len(first.history[p]) == first.results["rounds"][p] == len(first.fold_history[p][0]) <= 12
        assert first.history[p] == [a + b for a, b in zip(*first.fold_history[p])]
        best = first.results["best_iteration"][p]
        assert first.results["error"][p] == min(first.history[p]) == first.history[p][best]
        assert first.results["fold_errors"][p] == [curve[best] for curve in first.fold_history[p]]
    assert first.best_parameters == first.parameters[first.chosen]
    assert first.results["error"][first.chosen] == first.results["error"].min()
    assert same_result(first, ds.cross_validate(x, y, GRID, models_per_batch=4, **call))     # 2K
    assert same_result(first, ds.cross_validate(x, y, GRID, models_per_batch=None, **call))  # sized from the free HBM
    assert same_result(first, ds.cross_validate(x, y, GRID, models_per_batch=2, **call))     # the same call again
    assert {"cuts", "bin", "boost", "refit", "total"} <= set(first.timings)
    single = ds.cross_validate(x, y, GRID[1], refit=False, **call)             # one dict, no refit
    assert single.model is None and single.history[0] == first.history[1]


# ---- 5. cross_validate end to end ---------------------------------------------------------------------------------------
def crafted_early_stopping_set(seed=5):
    """test_gpu_trainer.py's crafted set with its evaluation rows appended.  Region A (x0 > 0, x1 < 0) is all positive,
    region B (x0 > 0, x1 >= 0) 99 % positive: the out-of-fold error falls when A and then B cross p > 0.9 and rises
    again while the model closes in on B's negatives."""
    rng = np.random.RandomState(seed)
    x = rng.uniform(-1, 1, (20000, 2)).astype(np.float32)
    y = ((x[:, 0] > 0) & ((x[:, 1] < 0) | (rng.rand(20000) < 0.99))).astype(np.float32)
    ex = np.concatenate([np.column_stack([rng.uniform(0.1, 1, 40), rng.uniform(-1, -0.1, 40)]),
                         np.column_stack([rng.uniform(0.1, 1, 10), rng.uniform(0.1, 1, 10)])]).astype(np.float32)
    ey = np.concatenate([np.ones(40), np.zeros(10)]).astype(np.float32)
    return np.concatenate([x, ex]), np.concatenate([y, ey])


@pytest.mark.parametrize("eta", [0.1, 0.3])
def test_cross_validate_stops_by_the_summed_curve_and_refits_like_fit(eta):
    """At the default eta no row crosses p > 0.9 in the first ten rounds: the summed curve starts flat, its first
    minimum is round 0 and the set stops at round 10, as the rule says (the CPU oracle gives 15 flat rounds).  At eta 0.3
    the oracle's curve falls from round 5, has its minimum near round 10 and rises: the same checks on a real curve."""
    import doppel_speller_amd as ds
    x, y = crafted_early_stopping_set()
    parameters = dict(max_depth=2) if eta == 0.1 else dict(max_depth=2, eta=eta)
    cv = ds.cross_validate(x, y, parameters, n_folds=3, seed=1, num_boost_round=150, early_stopping_rounds=10)
    stepper = ds.ForestTrainerBatch().begin(x, y, cv.folds, [dict(parameters, held_out=k) for k in range(3)])
    for _ in range(150):
        stepper.step()
    summed = [sum(errors) for errors in zip(*stepper.history)]
    stepper.close()
    expected_best, stopped = 0, len(summed) - 1                 # xgboost's rule on the summed curve
    for round_, error in enumerate(summed):
        if error < summed[expected_best]:
            expected_best = round_
        if round_ - expected_best >= 10:
            stopped = round_
            break
    print("summed curve:", summed[:stopped + 1], "best", expected_best, "stopped", stopped)
    assert expected_best == int(np.argmin(summed[:stopped + 1]))
    assert stopped == expected_best + 10 < 149                  # it stops exactly 10 rounds after its first minimum
    if eta == 0.3:
        assert expected_best > 0 and max(summed[expected_best:stopped + 1]) > summed[expected_best] < summed[0], summed
    assert cv.best_iteration == cv.results["best_iteration"][0] == expected_best
    assert cv.results["rounds"][0] == stopped + 1 and cv.history[0] == summed[:stopped + 1]
    assert cv.results["error"][0] == summed[expected_best]
    assert [len(curve) for curve in cv.fold_history[0]] == [stopped + 1] * 3
    trainer = ds.ForestTrainer()
    model = trainer.fit(x, y, num_boost_round=expected_best + 1, **parameters)
    assert model.n_trees == cv.model.n_trees == expected_best + 1 and same_model(cv.model, model)


# ---- 8. tune_model_parameters -------------------------------------------------------------------------------------------
def test_tune_model_parameters_equals_cross_validate_on_the_host_sets():
    import doppel_speller_amd as ds
    from doppel_speller_amd import synth, tuning
    w = synth.make_workload(2000, 400, seed=21, query_seed=22)
    truth, train = synth._to_strings(w.t_flat, w.t_off), synth._to_strings(w.q_flat, w.q_off)
    ids = np.where(w.actual_row >= 0, w.title_id[np.maximum(w.actual_row, 0)], -1)
    grid = ds.parameter_grid(max_depth=[2, 4], eta=[0.1, 0.3])
    call = dict(num_boost_round=30, early_stopping_rounds=30)
    tuned = ds.tune_model_parameters(truth, w.title_id, train, ids, grid, n_folds=3, top_n=10, sample_n=5, seed=9,
                                     transform=False, cover=True, **call)
    fe = ds.FeatureEngineering(truth, w.title_id, train, ids, top_n=10, sample_n=5, seed=9, transform=False,
                               evaluation_fractions=dict(generated=0.0, negative=0.0, positive=0.0))
    sets = fe.generate_device_data_sets()
    x, y, _, _ = sets.to_host()
    sets.free()
    assert x.shape == (len(fe.rows), 66) and tuned.rows.equals(fe.rows)
    groups = tuning.row_groups(fe.rows)
    host = ds.cross_validate(x, y, grid, n_folds=3, groups=groups, seed=9, **call)
    assert same_result(tuned, host)
    assert len(tuned.results) == 4 and (tuned.results["rounds"] == 30).all()
    keys = list(zip(fe.rows["kind"], fe.rows["query_index"]))
    fold_of = {}
    for key, f in zip(keys, tuned.folds.tolist()):
        assert fold_of.setdefault(key, f) == f                  # rows of one (kind, query_index) share a fold
    assert len(fold_of) < len(keys) and set(fold_of.values()) == {0, 1, 2}
    assert set(fe.timings) | {"cuts", "bin", "boost", "refit", "cover", "total"} <= set(tuned.timings)
    assert tuned.feature_importance.tobytes() == host.model.feature_importance().tobytes()
    contributions = tuned.model.predict_contributions(x[:50])
    assert contributions.shape == (50, 67)
    assert np.allclose(contributions.sum(axis=1), tuned.model.predict(x[:50], output_margin=True), atol=1e-4)
