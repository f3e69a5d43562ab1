"""Per-round metrics of ForestTrainer, ForestTrainerBatch and cross_validate on the GPU ("Metrics"):
after every step the device's AUC integers equal the NumPy oracle's (tests/metrics_oracle.py) on the margins read back
at that round, the log-loss sums are within one quantum per row, and requesting metrics changes no tree."""
import numpy as np
import pytest

import metrics_oracle as oracle
from forest_train_oracle import make_data

pytestmark = pytest.mark.gpu
MODEL_KEYS = ("feature", "threshold", "yes", "no", "missing", "tree_offsets")
BOTH = ("auc", "logloss")


def same_model(a, b):
    return all(a.arrays[key].tobytes() == b.arrays[key].tobytes() for key in MODEL_KEYS)


@pytest.fixture(scope="module")
def data():
    x, y = make_data(5000, 12, 61)
    ex, ey = make_data(2000, 12, 62)
    return x, y, ex, ey


def check_set(counts, margins, labels, beta, metrics, where):
    """One set's six integers against the oracle on its margins."""
    if "auc" in metrics:
        assert counts[:4] == oracle.auc_counts(margins, labels)[:4], where
    else:
        assert counts[:4] == (-1, -1, -1, -1), where
    if "logloss" in metrics:
        expected, rows = oracle.logloss_counts(margins, labels, beta)
        assert counts[5] == rows == margins.shape[0], where
        assert abs(counts[4] - expected) <= rows, (where, counts[4], expected)
    else:
        assert counts[4:] == (-1, -1), where


def step_and_check(trainer, y, ey, rounds, metrics, beta=5.0):
    heaps = []
    for round_ in range(rounds):
        trainer.step()
        heaps.append((trainer.last_heap[0].tobytes(), trainer.last_heap[1].tobytes()))
        counts = trainer.metric_counts[round_]
        check_set(counts["train"], trainer.margins(), y, beta, metrics, ("train", round_))
        if ey is not None:
            check_set(counts["evaluation"], trainer.eval_margins(), ey, beta, metrics, ("evaluation", round_))
        for set_ in counts:
            if "auc" in metrics:
                assert trainer.metrics_history[f"{set_}-auc"][round_] == oracle.auc(counts[set_])
            if "logloss" in metrics:
                assert trainer.metrics_history[f"{set_}-logloss"][round_] == oracle.logloss(counts[set_][4:])
    return heaps


@pytest.mark.parametrize("sampling", [{}, dict(subsample=0.5, colsample_bytree=0.5, sample_seed=3)], ids=["all", "sampled"])
def test_single_trainer_against_the_oracle_and_the_plain_run(data, sampling):
    """5,000 + 2,000 rows, 12 features, depth 3, 6 rounds in step form.  With subsample < 1 the training metrics still
    cover every training row: the oracle sees margins() of all of them."""
    import doppel_speller_amd as ds
    x, y, ex, ey = data
    trainer = ds.ForestTrainer().begin(x, y, ex, ey, max_depth=3, eval_metrics=BOTH, **sampling)
    heaps = step_and_check(trainer, y, ey, 6, BOTH)
    assert sorted(trainer.metrics_history) == ["evaluation-auc", "evaluation-logloss", "train-auc", "train-logloss"]
    assert all(len(curve) == 6 for curve in trainer.metrics_history.values())
    assert trainer.metrics_history["evaluation-auc"][-1] > 0.5 and trainer.metrics_history["train-auc"][-1] > 0.5
    assert trainer.metrics_history["train-logloss"][-1] < trainer.metrics_history["train-logloss"][0]
    plain = ds.ForestTrainer().begin(x, y, ex, ey, max_depth=3, **sampling)
    for round_ in range(6):
        plain.step()
        assert (plain.last_heap[0].tobytes(), plain.last_heap[1].tobytes()) == heaps[round_], round_
    assert plain.history == trainer.history and plain.metrics_history == {} and plain.metric_counts == []
    assert plain.margins().tobytes() == trainer.margins().tobytes()
    assert plain.eval_margins().tobytes() == trainer.eval_margins().tobytes()
    # the library's refusals: unknown bits, and any change after the first step
    from doppel_speller_amd import _lib
    fresh = ds.ForestTrainer().begin(x[:100], y[:100], max_depth=2)
    assert _lib.lib().ds_trainer_set_metrics(fresh.handle, 4) == -1                       # DS_E_ARG
    assert b"unknown bits" in _lib.lib().ds_last_error()
    assert _lib.lib().ds_trainer_set_metrics(trainer.handle, 1) == -1
    assert b"before the first round" in _lib.lib().ds_last_error()
    assert _lib.lib().ds_trainer_set_metrics(plain.handle, 3) == -1
    for one in (trainer, plain, fresh):
        one.close()


def test_fit_keeps_its_model_history_and_best_iteration(data):
    import doppel_speller_amd as ds
    x, y, ex, ey = data
    call = dict(num_boost_round=6, early_stopping_rounds=3, max_depth=3)
    with_metrics, plain = ds.ForestTrainer(), ds.ForestTrainer()
    model = with_metrics.fit(x, y, ex, ey, eval_metrics=("auc",), **call)
    assert same_model(model, plain.fit(x, y, ex, ey, **call))
    assert with_metrics.history == plain.history and with_metrics.best_iteration == plain.best_iteration
    assert sorted(with_metrics.metrics_history) == ["evaluation-auc", "train-auc"]
    assert len(with_metrics.metrics_history["train-auc"]) == len(with_metrics.history)
    assert all(counts["train"][4:] == (-1, -1) for counts in with_metrics.metric_counts)
    with_metrics.close()
    plain.close()


def test_depth_one_gives_two_distinct_margins_and_no_evaluation_set_no_evaluation_keys(data):
    import doppel_speller_amd as ds
    x, y, _, _ = data
    for metrics in (("auc",), ("logloss",), BOTH):
        trainer = ds.ForestTrainer().begin(x, y, max_depth=1, eval_metrics=metrics)
        step_and_check(trainer, y, None, 2, metrics)
        assert sorted(trainer.metrics_history) == sorted(f"train-{name}" for name in metrics)
        assert sorted(trainer.metric_counts[0]) == ["train"]
        trainer.close()
    trainer = ds.ForestTrainer().begin(x, y, max_depth=1, eval_metrics=("auc",))
    trainer.step()
    margins = trainer.margins()
    low, high = np.unique(margins)                                          # two leaves: two values
    in_class = lambda value, label: int(np.count_nonzero((margins == value) & (y == label)))
    assert trainer.metric_counts[0]["train"][:4] == (
        in_class(high, 1) * in_class(low, 0), in_class(low, 1) * in_class(low, 0) + in_class(high, 1) * in_class(high, 0),
        int(np.count_nonzero(y)), int(np.count_nonzero(y == 0)))
    trainer.close()


def test_device_matrices_and_roc_auc_of_a_device_array(data):
    import doppel_speller_amd as ds
    from doppel_speller_amd import _lib
    x, y, ex, ey = data
    d_x, d_ex = _lib.DeviceArray.from_host(x), _lib.DeviceArray.from_host(ex)
    trainer = ds.ForestTrainer().begin_device(d_x, 5000, y, d_ex, 2000, ey, max_depth=3, eval_metrics=BOTH)
    step_and_check(trainer, y, ey, 2, BOTH)
    margins = trainer.eval_margins()
    d_margins = _lib.DeviceArray.from_host(margins)
    assert ds.roc_auc(d_margins, ey) == ds.roc_auc(margins, ey) == trainer.metrics_history["evaluation-auc"][-1]
    assert ds.auc_counts(d_margins, ey)[:4] == trainer.metric_counts[-1]["evaluation"][:4]
    for one in (d_x, d_ex, d_margins):
        one.free()
    trainer.close()


# ---- the batch ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batch_data():
    import doppel_speller_amd as ds
    x, y = make_data(6000, 12, 71)
    return x, y, ds.fold_assignment(None, 3, seed=2, n=6000)


SETS = [dict(max_depth=2), dict(max_depth=4, beta=2.0)]
MODELS = [dict(one, held_out=k) for one in SETS for k in range(3)]


def run_batch(batch_data, metrics):
    """5 rounds, the second set inactive after round 3 -> per round the heaps and (with metrics) the library's table."""
    import doppel_speller_amd as ds
    x, y, fold = batch_data
    batch = ds.ForestTrainerBatch().begin(x, y, fold, MODELS, metrics=metrics)
    record = []
    for round_ in range(5):
        active = np.array([True] * 3 + [round_ < 3] * 3)
        batch.step(active)
        table = batch._metric_counts.copy()
        for m in np.nonzero(active)[0]:
            held = fold == m % 3
            if metrics:
                assert batch.metric_counts[m][-1] == tuple(int(v) for v in table[m])
                check_set(batch.metric_counts[m][-1], batch.margins(m)[held], y[held], MODELS[m].get("beta", 5.0),
                          metrics, (m, round_))
        record.append(dict(table=table, heaps=[None if h is None else (h[0].tobytes(), h[1].tobytes())
                                               for h in batch.last_heap]))
    return batch, record


def test_batch_against_the_oracle_with_inactive_models_and_capped_grids(batch_data):
    from doppel_speller_amd import tuning
    batch, record = run_batch(batch_data, BOTH)
    for m in range(6):
        assert len(batch.metric_counts[m]) == (5 if m < 3 else 3)
        assert len(batch.metrics_history[m]["auc"]) == len(batch.metrics_history[m]["logloss"]) == len(batch.history[m])
        assert batch.metrics_history[m]["auc"][-1] == oracle.auc(batch.metric_counts[m][-1])
    for round_ in (3, 4):                                     # the inactive models' cached values stay
        assert np.array_equal(record[round_]["table"][3:], record[2]["table"][3:])
        assert not np.array_equal(record[round_]["table"][:3], record[2]["table"][:3])
    assert (record[4]["table"] >= 0).all()
    batch.close()
    plain, plain_record = run_batch(batch_data, ())
    assert [r["heaps"] for r in plain_record] == [r["heaps"] for r in record]
    assert plain.metric_counts == [[] for _ in MODELS] and plain.history == batch.history
    plain.close()
    try:
        tuning.batch_option("max_blocks", 2)
        capped, capped_record = run_batch(batch_data, BOTH)
    finally:
        tuning.batch_option("max_blocks", 0)
    for a, b in zip(capped_record, record):
        assert np.array_equal(a["table"], b["table"]) and a["heaps"] == b["heaps"]
    capped.close()


def test_batch_refusals_and_a_model_without_a_fold(batch_data):
    import doppel_speller_amd as ds
    from doppel_speller_amd import _lib, tuning
    x, y, fold = batch_data
    batch = ds.ForestTrainerBatch().begin(x, y, fold, [dict(max_depth=2, held_out=-1), dict(max_depth=2, held_out=1)],
                                          metrics=("auc",))
    assert _lib.lib().ds_trainer_batch_set_metrics(batch.handle, 8) == -1
    batch.step()
    assert batch.metric_counts[0] == [(-1,) * 6] and batch.metrics_history[0]["auc"] == [None]
    held = fold == 1
    assert batch.metric_counts[1][0][:4] == oracle.auc_counts(batch.margins(1)[held], y[held])[:4]
    assert _lib.lib().ds_trainer_batch_set_metrics(batch.handle, 1) == -1
    assert b"before the first step" in _lib.lib().ds_last_error()
    batch.close()
    assert tuning.batch_metrics_bytes(6000, 6, 3) >= 4 * 6000 + 6 * 8 * 2000
    assert tuning.batch_metrics_bytes(0, 6, 3) == -1 and tuning.batch_metrics_bytes(6000, 257, 3) == -1


# ---- cross_validate -----------------------------------------------------------------------------------------------------
def test_cross_validate_reports_pooled_metrics_and_selects_by_them(batch_data):
    import doppel_speller_amd as ds
    from doppel_speller_amd.tuning import pooled_counts
    x, y, fold = batch_data
    call = dict(n_folds=3, seed=2, num_boost_round=8, early_stopping_rounds=3)
    by_auc = ds.cross_validate(x, y, SETS, metrics=("auc",), select_by="auc", refit=False, **call)
    assert np.array_equal(by_auc.folds, fold) and by_auc.select_by == "auc"
    assert list(by_auc.results.columns)[-1] == "auc" and "logloss" not in by_auc.results
    for p in range(2):
        rounds = by_auc.results["rounds"][p]
        assert len(by_auc.metrics_history[p]["auc"]) == rounds == len(by_auc.fold_metric_counts[p][0])
        for r in range(rounds):
            c, t, pairs, _, _ = pooled_counts([by_auc.fold_metric_counts[p][k][r] for k in range(3)])
            assert by_auc.metrics_history[p]["auc"][r] == (2 * c + t) / (2 * pairs)
            assert pairs == sum(int(np.count_nonzero(y[fold == k])) * int(np.count_nonzero(y[fold == k] == 0))
                                for k in range(3))
        assert by_auc.results["auc"][p] == by_auc.metrics_history[p]["auc"][by_auc.results["best_iteration"][p]]
        assert by_auc.results["auc"][p] == max(by_auc.metrics_history[p]["auc"])
    replayed = ds.select_parameters(by_auc.fold_history, 3, select_by="auc", metric_counts=by_auc.fold_metric_counts)
    assert replayed["chosen"] == by_auc.chosen and replayed["best_iteration"] == list(by_auc.results["best_iteration"])
    assert by_auc.best_iteration == replayed["best_iteration"][replayed["chosen"]]
    assert replayed["rounds"] == list(by_auc.results["rounds"])
    # select_by="error" with metrics: today's result in every field it has today, plus the reports
    today = ds.cross_validate(x, y, SETS, **call)
    reported = ds.cross_validate(x, y, SETS, metrics=BOTH, **call)
    columns = list(today.results.columns)
    assert columns == ["max_depth", "eta", "min_child_weight", "reg_lambda", "beta", "best_iteration", "error", "rounds",
                       "fold_errors"] and list(reported.results.columns) == columns + ["auc", "logloss"]
    assert reported.results[columns].equals(today.results)
    assert reported.history == today.history and reported.fold_history == today.fold_history
    assert reported.chosen == today.chosen and reported.best_iteration == today.best_iteration
    assert reported.best_parameters == today.best_parameters and reported.folds.tobytes() == today.folds.tobytes()
    assert same_model(reported.model, today.model)
    assert not hasattr(today, "metrics_history") and reported.select_by == "error"
    assert all(0.0 < value < 5.0 for value in reported.results["logloss"])
