"""Prediction.threshold_sweep and Prediction.evaluate on the GPU, on the synthetic truth set of the ranked tests (20,000
titles) and 400 titles, 40 % of them with no match: every checked cell against predictions_accuracy on what
generate_test_predictions answers with that cell's thresholds, and the variants that must not change the frame."""
import numpy as np
import pytest

import doppel_speller_amd as ds
from doppel_speller_amd import prediction, synth

pytestmark = pytest.mark.gpu

TOP_N = 10
LEVENSHTEIN = [80, 94, 97]


@pytest.fixture(scope="module")
def problem():
    """Truth titles under permuted ids, 400 queries (60 % misspelled truth titles, 20 of them verbatim ones) and the id
    each should get (-1: a fresh title), a forest, and probability thresholds laid between (one of them: on) the model's
    own maxima for the titles it decides, so that the model stage decides differently from cell to cell."""
    w = synth.make_workload(20000, 400)
    truth = synth._to_strings(w.t_flat, w.t_off)
    ids = w.title_id
    queries = synth._to_strings(w.q_flat, w.q_off)
    actual_row = w.actual_row.copy()
    rng = np.random.RandomState(5)
    for q in rng.permutation(400)[:20]:
        actual_row[q] = rng.randint(0, 20000)
        queries[q] = truth[actual_row[q]]
    actual = np.where(actual_row >= 0, ids[np.maximum(actual_row, 0)], -1).astype(np.int64)
    forest = synth.make_forest(n_trees=100)
    model = ds.ForestModel(forest["feature"], forest["threshold"], forest["yes"], forest["no"], forest["missing"],
                           forest["tree_offsets"], forest["n_features"], forest["base_margin"])
    p = ds.Prediction(truth, ids, model, top_n=TOP_N, transform=False)
    p.ranked_matches(queries, n=1, keep_candidates=True)
    undecided = (p.candidates.exact < 0) & (p.candidates.close < 0)
    maxima = np.unique(p.candidates.probabilities[undecided].max(axis=1))
    assert maxima.shape[0] >= 8
    cuts = [float((maxima[at] + maxima[at + 1]) / 2) for at in (len(maxima) // 4, len(maxima) // 2)]
    return truth, ids, queries, actual, model, sorted(cuts + [0.9, float(maxima[len(maxima) // 3])])


@pytest.fixture(scope="module")
def swept(problem):
    truth, ids, queries, actual, model, probabilities = problem
    p = ds.Prediction(truth, ids, model, top_n=TOP_N, transform=False)
    frame = p.threshold_sweep(queries, actual, LEVENSHTEIN, probabilities)
    return p, frame, dict(p.timings)


def _same_frame(a, b):
    return list(a.columns) == list(b.columns) and a.dtypes.tolist() == b.dtypes.tolist() and all(
        np.array_equal(a[c].to_numpy(), b[c].to_numpy()) for c in a.columns)


def _line(frame, t, u):
    line = frame[(frame["levenshtein_threshold"] == t) & (frame["probability_threshold"] == u)]
    assert len(line) == 1, (t, u)
    return {name: int(line.iloc[0][name]) for name in prediction.SWEEP_COLUMNS[2:]}


def test_the_frame(problem, swept):
    _, _, queries, _, _, probabilities = problem
    p, frame, timings = swept
    assert tuple(frame.columns) == prediction.SWEEP_COLUMNS and len(frame) == 3 * 4
    assert frame["levenshtein_threshold"].tolist() == sorted(LEVENSHTEIN * 4)
    assert frame["probability_threshold"].tolist() == probabilities * 3
    counts = frame[list(prediction.SWEEP_COLUMNS[2:6])].to_numpy()
    assert (counts.sum(axis=1) == len(queries)).all() and (counts >= 0).all()
    assert np.array_equal(frame["custom_error"].to_numpy(), counts[:, 3] + 5 * counts[:, 1])
    assert (counts.max(axis=0) > 0).all() and len(np.unique(counts, axis=0)) >= 3      # the cells differ
    assert {"top_k", "close_parts", "exact_matches", "features", "model", "sweep", "copy_back", "host_prepare",
            "prepare_queries"} == set(timings)
    assert timings["close_parts"] > 0 and timings["sweep"] > 0
    assert p.details is None and p.candidates is None


@pytest.mark.parametrize("t, u_index", [(94, None), (80, 0), (97, 0), (94, 3), (80, 3)])
def test_a_cell_is_the_accuracy_of_generate_test_predictions_there(problem, swept, t, u_index):
    """The parent's own answer: a Prediction built with the cell's thresholds, its title ids counted by
    predictions_accuracy.  u_index None: 0.9, the default."""
    truth, ids, queries, actual, model, probabilities = problem
    u = 0.9 if u_index is None else probabilities[u_index]
    p = ds.Prediction(truth, ids, model, top_n=TOP_N, transform=False, levenshtein_threshold=t, probability_threshold=u)
    answer = p.generate_test_predictions(queries)
    expected = ds.predictions_accuracy(answer["title_id"].to_numpy(), actual)
    assert _line(swept[1], t, u) == expected
    if (t, u) == (94, 0.9):
        assert p.evaluate(queries, actual) == expected
        assert {1, 2} <= set(p.details["stage"].tolist())             # the exact and the close stage decide some titles


def test_the_frame_does_not_depend_on_chunks_preparation_or_order(problem, swept):
    truth, ids, queries, actual, model, probabilities = problem
    p, frame, _ = swept
    for chunk in (150, 400, 1):
        p.chunk_queries = chunk
        for prepare in ("host", "device") if chunk != 1 else ("device",):
            p.prepare_queries = prepare
            assert _same_frame(frame, p.threshold_sweep(queries, actual, LEVENSHTEIN, probabilities)), (chunk, prepare)
            assert ("prepare_queries" in p.timings) == (prepare == "device")
    p.chunk_queries, p.prepare_queries = None, "device"
    # thresholds in any order, with repeats; the titles in any order under test indexes of the caller's
    order = np.random.RandomState(2).permutation(len(queries))
    shuffled = p.threshold_sweep([queries[i] for i in order], actual[order], LEVENSHTEIN[::-1] + [94],
                                 probabilities[::-1] + probabilities[:1], test_index=order + 1000)
    assert _same_frame(frame, shuffled)
    # None: the instance's own thresholds, one cell; evaluate reads it
    one = p.threshold_sweep(queries, actual)
    assert len(one) == 1 and _line(one, 94, 0.9) == _line(frame, 94, 0.9) == p.evaluate(queries, actual)
    empty = p.threshold_sweep([], [], LEVENSHTEIN, probabilities)
    assert len(empty) == 12 and not empty[list(prediction.SWEEP_COLUMNS[2:])].to_numpy().any()
    assert empty.dtypes.tolist() == frame.dtypes.tolist() and p.timings["sweep"] == 0.0
    with pytest.raises(ValueError, match="actual title id 20000 is neither"):
        p.threshold_sweep(queries[:2], [int(ids[0]), 20000])
