"""Metrics without a GPU ("Metrics"): the NumPy oracle of the rule against a brute-force count, the
checks of `eval_metrics`, `metrics` and `select_by` before any library call, and select_parameters on hand-made curves."""
import math

import numpy as np
import pytest

import metrics_oracle as oracle
from doppel_speller_amd import _lib

X = np.arange(36, dtype=np.float32).reshape(12, 3)
Y = (np.arange(12) % 2).astype(np.float32)


@pytest.fixture
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the library was called before the arguments were validated")
    monkeypatch.setattr(_lib, "lib", refuse)


# ---- the oracle itself --------------------------------------------------------------------------------------------------
def test_oracle_counts_equal_the_brute_force_count():
    """200 rows, heavy ties (12 distinct values), both zeros, both infinities and a NaN in either class."""
    rng = np.random.RandomState(5)
    scores = rng.choice(np.linspace(-3, 3, 12), 200).astype(np.float32)
    labels = (rng.rand(200) < 0.4).astype(np.float32)
    scores[:8] = [-0.0, 0.0, 0.0, -0.0, np.inf, -np.inf, np.inf, -np.inf]
    labels[:8] = [1, 0, 1, 0, 1, 0, 0, 1]
    scores[8], labels[8] = np.nan, 1
    scores[9], labels[9] = np.nan, 0
    got, brute = oracle.auc_counts(scores, labels), oracle.auc_counts_brute(scores, labels)
    assert got == brute
    assert got[4] == 2 and got[2] == np.count_nonzero(labels) - 1 and got[3] == 200 - np.count_nonzero(labels) - 1
    assert got[1] > 100                                      # the ties are heavy
    # the zeros tie across their signs, and the order is the floats' own
    assert oracle.auc_counts(np.float32([-0.0, 0.0]), [1, 0])[:2] == (0, 1)
    assert oracle.auc_counts(np.float32([-np.inf, -1e-45, 0.0, 1e-45, np.inf]), [0, 1, 0, 1, 0])[:2] == (3, 0)
    floats = np.sort(rng.randn(500).astype(np.float32))
    assert np.array_equal(np.argsort(oracle.keys(floats), kind="stable"), np.arange(500))


def test_oracle_logloss_rule():
    margins = np.float32([0.0, 0.0, 30.0, -30.0, 5000.0, -5000.0, np.nan])
    labels = np.float32([1, 0, 0, 1, 0, 1, 1])
    terms = oracle.logloss_terms(margins, labels, 5.0)
    assert terms[0] == round(math.log(2.0) * (1 << 20)) and terms[1] == round(5 * math.log(2.0) * (1 << 20))
    assert terms[2] == 150 << 20 and terms[3] == 30 << 20                    # beta * softplus(30), softplus(30)
    assert terms[4] == terms[5] == terms[6] == 2048 << 20                    # the cap, for a NaN too
    assert oracle.logloss_counts(margins, labels, 5.0) == (int(terms.sum()), 7)
    # an infinite margin: no loss on the row's own side, the cap on the other
    assert oracle.logloss_terms(np.float32([np.inf, -np.inf, np.inf, -np.inf]), [1, 0, 0, 1], 5.0).tolist() == \
        [0, 0, 2048 << 20, 2048 << 20]


def test_oracle_logloss_against_the_probability_form():
    """The same loss written the textbook way, -(y log p + beta (1 - y) log(1 - p)) with p = 1 / (1 + exp(-m)) in
    float64, and -- for finite margins -- as the literal sum of both products: margins in [-10, 10], where 1 - p keeps
    its digits, agree within one quantum; the literal sum agrees exactly at every finite margin."""
    rng = np.random.RandomState(12)
    margins = rng.uniform(-10, 10, 4000).astype(np.float32)
    labels = (rng.rand(4000) < 0.5).astype(np.float64)
    m = margins.astype(np.float64)
    p = 1.0 / (1.0 + np.exp(-m))
    textbook = -(labels * np.log(p) + 5.0 * (1.0 - labels) * np.log1p(-p))
    terms = oracle.logloss_terms(margins, labels, 5.0).astype(np.int64)
    assert np.abs(terms - np.rint(textbook * (1 << 20)).astype(np.int64)).max() <= 1
    wide = np.concatenate([margins * 40, np.float32([0.0, -0.0, 1e-30, -1e-30, 3e38, -3e38])])
    wide_labels = np.concatenate([labels, [1, 0, 1, 0, 1, 0]])
    w = wide.astype(np.float64)
    literal = wide_labels * oracle.softplus(-w) + 5.0 * (1.0 - wide_labels) * oracle.softplus(w)
    assert np.array_equal(oracle.logloss_terms(wide, wide_labels, 5.0),
                          np.rint(np.fmin(literal, 2048.0) * (1 << 20)).astype(np.uint64))


def test_an_empty_class_gives_nan(monkeypatch):
    from doppel_speller_amd import train
    assert math.isnan(train.auc_value((0, 0, 0, 5, 0))) and math.isnan(train.auc_value((0, 0, 5, 0, 0)))
    assert train.auc_value((3, 2, 2, 2, 0)) == 1.0
    monkeypatch.setattr(train, "auc_counts", lambda scores, target, device=0: oracle.auc_counts(scores, target))
    assert math.isnan(train.roc_auc(np.float32([1, 2, 3]), [1, 1, 1]))
    assert math.isnan(train.roc_auc(np.float32([1, 2, 3]), [0, 0, 0]))
    assert train.roc_auc(np.float32([1, 2, 3, 3]), [0, 0, 1, 0]) == oracle.auc((2, 1, 1, 3, 0)) == 5 / 6
    assert train.logloss_value((0, 0, 1, 1, 3 << 20, 2)) == 1.5 and math.isnan(train.logloss_value((-1, -1, 0, 0)))


# ---- validation ---------------------------------------------------------------------------------------------------------
def test_eval_metrics_are_validated(no_library):
    import doppel_speller_amd as ds
    from doppel_speller_amd import train
    assert train.validate_parameters()["eval_metrics"] == ()
    assert train.validate_parameters(eval_metrics=("auc",))["eval_metrics"] == ("auc",)
    assert train.validate_parameters(eval_metrics=["logloss", "auc"])["eval_metrics"] == ("auc", "logloss")
    assert train.validate_fit(X, Y, eval_metrics=("logloss",))[4]["eval_metrics"] == ("logloss",)
    device = _lib.DeviceArray.view(4096, (12, 3), np.float32, 0)      # never read: the checks come first
    for bad in (("rmse",), "auc", ("auc", "auc"), ("auc", 3), None, {"auc": 1}, 7):
        for call in (lambda: train.validate_parameters(eval_metrics=bad),
                     lambda: train.validate_fit(X, Y, eval_metrics=bad),
                     lambda: train.validate_fit_device(device, 12, Y, eval_metrics=bad),
                     lambda: ds.ForestTrainer().begin(X, Y, eval_metrics=bad),
                     lambda: ds.ForestTrainer().fit(X, Y, eval_metrics=bad),
                     lambda: ds.ForestTrainer().begin_device(device, 12, Y, eval_metrics=bad),
                     lambda: ds.ForestTrainer().fit_device(device, 12, Y, eval_metrics=bad),
                     lambda: ds.train_model(["alpha beta", "gamma delta"], [5, 6], ["alpha bet"], [5], top_n=2,
                                            sample_n=1, eval_metrics=bad),
                     lambda: ds.ForestTrainerBatch().begin(X, Y, np.arange(12) % 3, [dict(held_out=0)], metrics=bad)):
            with pytest.raises(ValueError, match="eval_metrics|metrics"):
                call()


def test_cross_validation_refuses_bad_metrics_before_the_library(no_library):
    import doppel_speller_amd as ds
    from doppel_speller_amd import tuning
    titles = (["alpha beta", "gamma delta"], [5, 6], ["alpha bet", "unknown"], [5, -1])
    for arguments, message in ((dict(metrics=("rmse",)), "metrics holds 'rmse'"),
                               (dict(metrics="auc"), "metrics must be a tuple"),
                               (dict(metrics=("auc", "auc")), "twice"),
                               (dict(select_by="auc"), "needs that metric"),
                               (dict(metrics=("logloss",), select_by="auc"), "needs that metric"),
                               (dict(metrics=("auc",), select_by="rmse"), "select_by must be one of"),
                               (dict(metrics=("auc",), select_by=None), "select_by must be one of")):
        for call in (lambda: tuning.validate_cross_validation(dict(max_depth=2), 3, **arguments),
                     lambda: ds.cross_validate(X, Y, dict(max_depth=2), n_folds=3, **arguments),
                     lambda: ds.tune_model_parameters(*titles, dict(max_depth=2), n_folds=2, top_n=2, sample_n=1,
                                                      **arguments)):
            with pytest.raises(ValueError, match=message):
                call()
    assert tuning.validate_cross_validation(dict(max_depth=2), 3, metrics=("logloss", "auc"), select_by="logloss")[1] \
        is None
    assert tuning.validate_selection(["logloss", "auc"], "auc") == (("auc", "logloss"), "auc")


# ---- select_parameters on hand-made curves ----------------------------------------------------------------------------
def counts(concordant, ties=0, logloss_sum=-1, positives=10, negatives=10, rows=20):
    return (concordant, ties, positives, negatives, logloss_sum, rows if logloss_sum >= 0 else -1)


def test_select_by_auc_takes_the_first_maximum_and_stops_early_on_it():
    from doppel_speller_amd import select_parameters
    from doppel_speller_amd.tuning import pooled_counts, pooled_values
    # two folds per set; the pooled AUC numerators sum(2 c + t) per round:
    #   set 0: 100, 140, 140, 120, 110, 150 -> the first maximum within 3 rounds of patience is round 1 (140); round 5
    #          (150) lies beyond the stop at round 4
    #   set 1: 100, 120, 139, 130 -> best 139 at round 2
    errors = [[[9, 8, 7, 6, 5, 4], [9, 8, 7, 6, 5, 4]], [[1, 1, 1, 1], [1, 1, 1, 1]]]
    auc = [[[counts(20, 10), counts(30, 10), counts(35, 0), counts(30, 0), counts(25, 5), counts(40, 0)],
            [counts(25, 0), counts(35, 0), counts(35, 0), counts(30, 0), counts(25, 5), counts(35, 0)]],
           [[counts(25, 0), counts(30, 0), counts(35, 0), counts(30, 5)],
            [counts(25, 0), counts(30, 0), counts(34, 1), counts(30, 5)]]]
    out = select_parameters(errors, 3, select_by="auc", metric_counts=auc)
    assert out["best_iteration"] == [1, 2] and out["rounds"] == [5, 4]
    assert out["score"] == [-140, -139] and out["chosen"] == 0
    assert out["error"] == [16, 2]                              # the summed error AT the chosen rounds, not its minimum
    assert out["history"] == [[18, 16, 14, 12, 10], [2, 2, 2, 2]]
    assert out["metrics_history"][0]["auc"] == [100 / 400, 140 / 400, 140 / 400, 120 / 400, 110 / 400]
    assert out["metrics_history"][1]["auc"][2] == 139 / 400 and "logloss" not in out["metrics_history"][0]
    # without early stopping the later, higher maximum is found
    late = select_parameters(errors, None, select_by="auc", metric_counts=auc)
    assert late["best_iteration"] == [5, 2] and late["score"] == [-150, -139]
    # the same curves judged by the error choose the other set; the metrics are only reported
    by_error = select_parameters(errors, 3, metric_counts=auc)
    assert by_error["chosen"] == 1 and by_error["error"] == [8, 2] and by_error["best_iteration"] == [5, 0]
    assert "score" not in by_error and len(by_error["metrics_history"][0]["auc"]) == 6
    # a tie of the AUC numerators goes to the smaller best_iteration, then to the earlier set
    tie = select_parameters([[[3, 3]], [[3, 3]], [[3, 3]]], None, select_by="auc",
                            metric_counts=[[[counts(5), counts(9)]], [[counts(9), counts(9)]], [[counts(9), counts(1)]]])
    assert tie["best_iteration"] == [1, 0, 0] and tie["chosen"] == 1
    # pooling is by integer sums, whatever the order of the folds
    folds = [counts(7, 3, 5 << 20, 4, 6, 10), counts(50, 0, 1 << 20, 10, 9, 19), counts(0, 1, 0, 1, 1, 2)]
    assert pooled_counts(folds) == pooled_counts(folds[::-1]) == (57, 4, 24 + 90 + 1, 6 << 20, 31)
    assert pooled_values(pooled_counts(folds)) == {"auc": 118 / 230, "logloss": 6 / 31}


def test_select_by_logloss_minimises_the_integer_sum():
    from doppel_speller_amd import select_parameters
    loss = [[[counts(-1, -1, 900), counts(-1, -1, 700), counts(-1, -1, 800)],
             [counts(-1, -1, 100), counts(-1, -1, 200), counts(-1, -1, 50)]],
            [[counts(-1, -1, 500), counts(-1, -1, 400), counts(-1, -1, 400)],
             [counts(-1, -1, 500), counts(-1, -1, 449), counts(-1, -1, 449)]]]
    errors = [[[5, 5, 5], [5, 5, 5]], [[6, 6, 6], [6, 6, 6]]]
    out = select_parameters(errors, None, select_by="logloss", metric_counts=loss)
    assert out["score"] == [850, 849] and out["best_iteration"] == [2, 1] and out["chosen"] == 1
    assert out["metrics_history"][1] == {"logloss": [1000 / (1 << 20) / 40, 849 / (1 << 20) / 40, 849 / (1 << 20) / 40]}
    with pytest.raises(ValueError, match="do not hold that metric"):
        select_parameters(errors, None, select_by="auc", metric_counts=loss)


def test_error_ties_are_resolved_as_before():
    from doppel_speller_amd import select_parameters
    histories = [[[4, 3, 3], [4, 2, 2]], [[3, 3, 9], [2, 2, 9]], [[5, 5, 5], [0, 0, 0]]]
    plain = select_parameters(histories)
    assert plain == select_parameters(histories, None, select_by="error") == select_parameters(histories, None, "error", None)
    assert plain["error"] == [5, 5, 5] and plain["best_iteration"] == [1, 0, 0] and plain["chosen"] == 1
    assert set(plain) == {"chosen", "best_iteration", "error", "rounds", "history"}


def test_select_by_an_unrequested_metric_raises():
    from doppel_speller_amd import select_parameters
    with pytest.raises(ValueError, match="needs that metric"):
        select_parameters([[[1, 2]]], None, select_by="auc")
    with pytest.raises(ValueError, match="needs that metric"):
        select_parameters([[[1, 2]]], None, select_by="logloss", metric_counts=None)
    with pytest.raises(ValueError, match="select_by must be one of"):
        select_parameters([[[1, 2]]], None, select_by="rmse")
    with pytest.raises(ValueError, match="shape of the folds' curves"):
        select_parameters([[[1, 2]]], None, metric_counts=[[[counts(1)]]])


def test_abi_surface():
    assert {"ds_auc_device", "ds_auc", "ds_weighted_logloss_device", "ds_metrics_option", "ds_trainer_set_metrics",
            "ds_trainer_metrics", "ds_trainer_batch_set_metrics", "ds_trainer_batch_metrics",
            "ds_trainer_batch_metrics_bytes"} <= set(_lib.EXPORTED_SYMBOLS)
    assert "ds_metrics.hip" in _lib._SOURCES
    import doppel_speller_amd as ds
    assert callable(ds.roc_auc) and callable(ds.auc_counts)
