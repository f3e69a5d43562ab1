"""Calibration through the public surface on the GPU: ForestModel.calibrate against fit_isotonic of predict, the
calibrated_probability column of ranked_matches, exhaustive_matches and explain against the oracle's map
(tests/calibration_oracle.py) of their probability column, raw_threshold as a probability_threshold of
generate_test_predictions, and train_model(calibrate=True).  A model of a handful of random trees, 600 truth titles and
60 queries."""
import numpy as np
import pytest

import calibration_oracle as oracle

pytestmark = pytest.mark.gpu


def _bits(values):
    return np.ascontiguousarray(values).tobytes()


@pytest.fixture(scope="module")
def problem():
    """600 truth titles, 60 queries (12 of them verbatim truth titles), 8 random trees with a counted cover, and a
    calibrator fitted on 3,000 random rows whose labels follow the model's probability."""
    import doppel_speller_amd as ds
    from doppel_speller_amd import synth
    w = synth.make_workload(600, 60, seed=41)
    truth = synth._to_strings(w.t_flat, w.t_off)
    queries = synth._to_strings(w.q_flat, w.q_off)
    rng = np.random.RandomState(42)
    for q, t in zip(rng.permutation(60)[:12], rng.randint(0, 600, 12)):
        queries[q] = truth[t]
    forest = synth.make_forest(seed=43, n_trees=8)
    model = ds.ForestModel(forest["feature"], forest["threshold"], forest["yes"], forest["no"], forest["missing"],
                           forest["tree_offsets"], forest["n_features"], forest["base_margin"])
    rows = rng.uniform(0, 100, (3000, forest["n_features"])).astype(np.float32)     # the scale of the forest's cuts
    rows[rng.rand(*rows.shape) < 0.3] = np.nan
    model.fit_cover(rows, prior=1.0)
    p = model.predict(rows).astype(np.float64)
    target = (rng.random_sample(3000) < (p - p.min()) / (p.max() - p.min())).astype(np.float32)
    calibrator = model.calibrate(rows, target)
    return dict(truth=truth, ids=np.asarray(w.title_id, dtype=np.int64), queries=queries, model=model, rows=rows,
                target=target, calibrator=calibrator)


def _expected(calibrator, probability):
    return oracle.transform(calibrator.lo, calibrator.values, np.asarray(probability, dtype=np.float32))


def _same_shared_columns(with_column, without):
    assert [c for c in with_column.columns if c != "calibrated_probability"] == list(without.columns)
    at = list(with_column.columns).index("calibrated_probability")
    assert with_column.columns[at - 1] == "probability" and with_column["calibrated_probability"].dtype == np.float32
    for column in without.columns:
        assert with_column[column].dtype == without[column].dtype
        assert _bits(with_column[column].to_numpy()) == _bits(without[column].to_numpy()), column


def test_calibrate_is_the_fit_of_predict(problem):
    import doppel_speller_amd as ds
    model, rows, target, c = (problem[k] for k in ("model", "rows", "target", "calibrator"))
    probabilities = model.predict(rows)
    assert c == ds.fit_isotonic(probabilities, target)
    want = oracle.fit(probabilities, target)
    assert c == ds.Calibrator(want["lo"], want["hi"], want["pos"], want["neg"], want["n_nan"])
    assert len(c) >= 2 and c.kind == "probability" and c.n_rows == 3000 and c.n_nan == 0
    assert model.calibrate(rows[:0], target[:0]) == ds.Calibrator([], [], [], [])


def test_the_frames_gain_one_column_and_nothing_else_changes(problem):
    import doppel_speller_amd as ds
    from doppel_speller_amd import prediction
    truth, ids, queries, model, c = (problem[k] for k in ("truth", "ids", "queries", "model", "calibrator"))
    plain = ds.Prediction(truth, ids, model, top_n=10, transform=False)
    mapped = ds.Prediction(truth, ids, model, top_n=10, transform=False, calibrator=c, chunk_queries=25)

    before, after = plain.ranked_matches(queries, n=4), mapped.ranked_matches(queries, n=4)
    assert tuple(before.columns) == prediction.RANKED_COLUMNS and "calibrate" not in plain.timings
    assert "calibrate" in mapped.timings and mapped.timings["calibrate"] > 0
    _same_shared_columns(after, before)
    want = np.where(after["stage"].to_numpy() == 3, _expected(c, after["probability"]), np.float32(1))
    assert _bits(after["calibrated_probability"].to_numpy()) == _bits(want.astype(np.float32))
    assert set(after["stage"].tolist()) >= {1, 3}

    before, after = plain.exhaustive_matches(queries, n=3), mapped.exhaustive_matches(queries, n=3)
    assert tuple(before.columns) == prediction.EXHAUSTIVE_COLUMNS and "calibrate" not in plain.timings
    _same_shared_columns(after, before)
    assert _bits(after["calibrated_probability"].to_numpy()) == _bits(_expected(c, after["probability"]))

    before, after = plain.explain(queries), mapped.explain(queries)
    assert tuple(before.columns) == prediction.EXPLAIN_COLUMNS and "calibrate" not in plain.timings
    _same_shared_columns(after, before)
    assert _bits(after["calibrated_probability"].to_numpy()) == _bits(_expected(c, after["probability"]))
    assert _bits(plain.contributions) == _bits(mapped.contributions)


def test_raw_threshold_decides_at_the_calibrated_level(problem):
    import doppel_speller_amd as ds
    truth, ids, queries, model, c = (problem[k] for k in ("truth", "ids", "queries", "model", "calibrator"))
    scorer = ds.Prediction(truth, ids, model, top_n=10, transform=False)
    scorer.ranked_matches(queries, n=1, keep_candidates=True)
    kept = scorer.candidates
    best = kept.probabilities.max(axis=1)
    single = (kept.probabilities == best[:, None]).sum(axis=1) == 1
    reaches_model = (kept.exact < 0) & (kept.close < 0)
    calibrated = _expected(c, best).astype(np.float64)
    levels = sorted({float(np.median(calibrated[reaches_model])), float(c.values32()[len(c) // 2])} - {0.0, 1.0})
    assert levels                                   # the middle block of two or more has a value above 0
    for q in levels:
        decider = ds.Prediction(truth, ids, model, top_n=10, transform=False, probability_threshold=c.raw_threshold(q))
        decider.generate_test_predictions(queries)
        accepted = decider.details["stage"].to_numpy() == 3
        assert np.array_equal(accepted, reaches_model & single & (calibrated > q)), q
        rows = kept.rows[np.arange(len(queries)), kept.probabilities.argmax(axis=1)]
        assert np.array_equal(decider.details["match_row"].to_numpy()[accepted], rows[accepted])


def test_train_model_calibrates_the_evaluation_set_and_trains_the_same_model():
    """300 truth titles, 56 train titles, top_n = 20."""
    import doppel_speller_amd as ds
    from doppel_speller_amd import synth
    w = synth.make_workload(300, 56, seed=31, query_seed=32)
    truth, train = synth._to_strings(w.t_flat, w.t_off), synth._to_strings(w.q_flat, w.q_off)
    ids = np.where(w.actual_row >= 0, w.title_id[np.maximum(w.actual_row, 0)], -1)
    data = dict(top_n=20, sample_n=4, seed=9, transform=False)
    fit = dict(num_boost_round=6, early_stopping_rounds=6, max_depth=3, eta=0.3)
    plain = ds.train_model(truth, w.title_id, train, ids, **data, **fit)
    off = ds.train_model(truth, w.title_id, train, ids, **data, **fit, calibrate=False)
    result = ds.train_model(truth, w.title_id, train, ids, **data, **fit, calibrate=True, reliability_bins=8)
    assert plain.calibrator is None and plain.reliability is None and plain.calibrated_reliability is None
    assert off.calibrator is None and off.timings.keys() == plain.timings.keys() and "calibration" not in off.timings
    assert "calibration" in result.timings
    for other in (off, result):
        assert all(_bits(other.model.arrays[k]) == _bits(plain.model.arrays[k]) for k in plain.model.arrays)
        assert other.history == plain.history and other.error_matrix == plain.error_matrix
    fe = ds.FeatureEngineering(truth, w.title_id, train, ids, **data)
    _, _, evaluation, evaluation_target = fe.generate_train_and_evaluation_data_sets()
    assert result.calibrator == result.model.calibrate(evaluation, evaluation_target)
    probabilities = result.model.predict(evaluation)
    want = oracle.fit(probabilities, evaluation_target)
    assert _bits(result.calibrator.pos) == _bits(want["pos"]) and _bits(result.calibrator.lo) == _bits(want["lo"])
    assert _bits(result.reliability.counts) == _bits(oracle.reliability(probabilities, evaluation_target, 8))
    mapped = oracle.transform(want["lo"], result.calibrator.values, probabilities)
    assert _bits(result.calibrated_reliability.counts) == _bits(oracle.reliability(mapped, evaluation_target, 8))
    assert result.calibrated_reliability.n == result.reliability.n == evaluation.shape[0]
