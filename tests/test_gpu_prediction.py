"""Prediction.generate_test_predictions on the GPU against the restatement of the reference's four stages built from the
CPU oracle in tests/prediction_restatement.py (predict.py:97-113 exact, :140-183 close, :185-254 model, :256-272
finalise); tests/test_reference_stages_cpu.py holds that restatement against answers captured from the reference."""
import numpy as np
import pytest

import doppel_speller_amd as ds
from doppel_speller_amd import synth
from prediction_restatement import Expected as _Expected

pytestmark = pytest.mark.gpu


def _problem():
    """20,000 truth titles (a few duplicated under new ids) and 2,000 queries, 10 % of them verbatim truth titles."""
    w = synth.make_workload(20000, 2000)
    truth = synth._to_strings(w.t_flat, w.t_off)
    ids = list(w.title_id)
    rng = np.random.RandomState(21)
    duplicated = rng.randint(0, 20000, 40)
    truth += [truth[i] for i in duplicated]
    ids += list(range(20000, 20040))
    queries = synth._to_strings(w.q_flat, w.q_off)
    verbatim = rng.permutation(2000)[:200]
    sources = np.concatenate((duplicated[:20], rng.randint(0, len(truth), 180)))
    for q, t in zip(verbatim, sources):
        queries[q] = truth[t]
    forest = synth.make_forest(n_trees=100)
    model = ds.ForestModel(forest["feature"], forest["threshold"], forest["yes"], forest["no"], forest["missing"],
                           forest["tree_offsets"], forest["n_features"], forest["base_margin"])
    return truth, np.array(ids, dtype=np.int64), queries, forest, model


@pytest.fixture(scope="module")
def problem():
    return _problem()


@pytest.mark.parametrize("k", [10, 100])
def test_generate_test_predictions_matches_the_restated_reference(problem, oracle, k):
    truth, ids, queries, forest, model = problem
    expected = _Expected(truth, queries, k, oracle)
    oracle_probabilities = oracle.forest_predict(forest, expected.features)[1]
    gpu_probabilities = model.predict(expected.features)          # the forest kernel on the same feature bits
    # a threshold between two per-query maxima so that the model stage decides some queries and leaves others
    maxima = np.unique(oracle_probabilities.reshape(-1, k).max(axis=1))
    at = int(0.8 * maxima.shape[0])
    threshold = float((maxima[at] + maxima[at + 1]) / 2)

    p = ds.Prediction(truth, ids, model, top_n=k, transform=False, probability_threshold=threshold)
    out = p.generate_test_predictions(queries)
    details = p.details
    assert list(out.columns) == ["title_id", "test_index"]
    assert out["test_index"].tolist() == list(range(len(queries)))
    stage = details["stage"].to_numpy()
    row = details["match_row"].to_numpy()
    assert {0, 1, 2, 3} <= set(stage.tolist()), np.bincount(stage)

    # exact and close stages: exactly the restatement
    assert np.array_equal(np.where(stage == 1, row, -1), expected.exact)
    assert np.array_equal(np.where(stage == 2, row, -1), np.where(expected.exact >= 0, -1, expected.close))
    # model stage: exactly select_matches on the GPU's own predictions
    model_rows = expected.model_rows(gpu_probabilities, threshold, oracle)
    assert np.array_equal(np.where(stage == 3, row, -1), model_rows)
    # against the fully oracle-driven answer: only near-ties of the deciding probability may differ
    oracle_rows = expected.model_rows(oracle_probabilities, threshold, oracle)
    differ = np.nonzero(model_rows != oracle_rows)[0]
    grouped = oracle_probabilities.reshape(-1, k)
    near = 0
    for q in differ:
        group = grouped[np.searchsorted(expected.pair_q[::k], q)]
        top = np.sort(group)[::-1]
        assert min(abs(top[0] - threshold), top[0] - top[1]) <= 1e-5, q
        near += 1
    assert near <= 0.005 * len(queries)
    print(f"top-{k}: stages {np.bincount(stage).tolist()}, {near} queries differ from the oracle-driven answer by a "
          f"probability within 1e-5 of the threshold or the runner-up")
    assert np.array_equal(out["title_id"].to_numpy(), np.where(row >= 0, ids[np.maximum(row, 0)], -1))

    if k == 100:
        for chunk in (None, 700):
            p.chunk_queries = chunk
            assert out.equals(p.generate_test_predictions(queries)), chunk
        subset = queries[:50]
        p.chunk_queries = None
        whole = p.generate_test_predictions(subset, test_index=np.arange(50)[::-1])
        p.chunk_queries = 1
        assert whole.equals(p.generate_test_predictions(subset, test_index=np.arange(50)[::-1]))
        assert whole["test_index"].tolist() == list(range(50))
        assert whole["title_id"].tolist() == out["title_id"].to_numpy()[:50][::-1].tolist()


def test_closest_search_single_title(problem, oracle):
    truth, ids, queries, forest, model = problem
    k = 10
    expected = _Expected(truth, queries, k, oracle)
    p = ds.Prediction(truth, ids, model, top_n=k, transform=False)
    gpu_probabilities = model.predict(expected.features).reshape(-1, k)

    q = int(np.nonzero(expected.exact >= 0)[0][0])
    found = p.closest_search_single_title("  " + queries[q] + " ")
    assert set(found) == {"test_index", "transformed_title", "match_transformed_title", "title_id", "prediction"}
    assert found["title_id"] == ids[expected.exact[q]] and found["prediction"] == 1.0
    assert found["match_transformed_title"] == queries[q]

    q = int(np.nonzero((expected.exact < 0) & (expected.close >= 0))[0][0])
    found = p.closest_search_single_title(queries[q])
    assert found["title_id"] == ids[expected.close[q]] and found["prediction"] == 1.0

    # the model: the best candidate with no threshold, the first in top-k order on a tie
    groups = expected.pair_q[::k]
    r = int(np.argmin(gpu_probabilities.max(axis=1)))              # a query far below any threshold
    q = int(groups[r])
    first_best = int(np.argmax(gpu_probabilities[r]))
    found = p.closest_search_single_title(queries[q])
    assert found["title_id"] == ids[expected.pair_t[r * k + first_best]]
    assert found["prediction"] == float(gpu_probabilities[r, first_best])
    assert p.details["stage"].tolist() == [3]
