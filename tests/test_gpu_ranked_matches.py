"""Prediction.ranked_matches on the GPU, on the problem of tests/test_gpu_prediction.py (rebuilt here): the intermediates
it keeps against the restated stages, the frame against the restated ranking rule (tests/ranked_cases.py) applied to
those intermediates, rank 1 against generate_test_predictions, and the variants that must not change the frame."""
import numpy as np
import pandas as pd
import pytest

import doppel_speller_amd as ds
import ranked_cases as rc
from doppel_speller_amd import prediction, synth
from doppel_speller_amd.match_maker import NativeProblem

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def problem():
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
    return truth, np.array(ids, dtype=np.int64), queries, model


class _Stages:
    """The stages before the model restated with the oracle: exact dict, Jaccard top-k, close ratios and rows."""

    def __init__(self, truth, queries, k, oracle):
        last = {}
        for row, title in enumerate(truth):
            last[title] = row
        self.exact = np.array([last.get(q, -1) for q in queries], dtype=np.int64)
        t_chars, t_offsets = prediction._pack(truth)
        q_chars, q_offsets = prediction._pack(queries)
        a = NativeProblem.from_flat(t_chars, t_offsets, q_chars, q_offsets, 3).arrays()
        self.rows = oracle.jaccard_topk(a["rowptr"], a["truth_idx"], a["idf32"], a["sums32"], a["q_rowptr"],
                                        a["q_cols"], a["q_maxint"], k)
        t_enc, t_len = ds.encode_titles(truth)
        self.q_enc, self.q_len = ds.encode_titles(queries)
        pair_q = np.repeat(np.arange(len(queries)), k)
        pair_t = self.rows.reshape(-1)
        self.ratios = oracle.close_ratios(self.q_len[pair_q], t_len[pair_t], self.q_enc[pair_q], t_enc[pair_t],
                                          ds.SPACE_CODE, ds.SORT_KEY, 94).reshape(-1, k)
        frame = pd.DataFrame({"q": pair_q, "t": pair_t, "ratio": self.ratios.reshape(-1).astype(np.int64)})
        frame = frame[frame["ratio"] > 94]                                              # predict.py:172
        frame = frame[frame.groupby("q")["ratio"].transform("max") == frame["ratio"]]    # :173-174
        frame = frame[~frame["q"].isin(frame.loc[frame["q"].duplicated(), "q"])]        # :176, :158-161
        self.close = np.full(len(queries), -1, dtype=np.int64)
        self.close[frame["q"].to_numpy()] = frame["t"].to_numpy()
        self.pair_q, self.pair_t = pair_q, pair_t


def _expected_frame(candidates, n, n_truth, test_index, ids):
    best = np.where(candidates.exact >= 0, candidates.exact, candidates.close)
    slots = rc.rank_matches(candidates.rows, candidates.probabilities, candidates.ratios, candidates.exact, best, n,
                            n_truth)
    return prediction.ranked_frame(test_index, *slots, ids)


def _same_frame(a, b):
    return list(a.columns) == list(b.columns) and a.dtypes.tolist() == b.dtypes.tolist() and all(
        np.array_equal(np.ascontiguousarray(a[c].to_numpy()).view(np.uint8),
                       np.ascontiguousarray(b[c].to_numpy()).view(np.uint8)) for c in a.columns)


@pytest.mark.parametrize("k", [10, 100])
def test_ranked_matches_against_the_restated_stages_and_rule(problem, oracle, k):
    truth, ids, queries, model = problem
    n_truth, n_queries = len(truth), len(queries)
    stages = _Stages(truth, queries, k, oracle)
    p = ds.Prediction(truth, ids, model, top_n=k, transform=False)
    frame = p.ranked_matches(queries, n=5, keep_candidates=True)
    c = p.candidates
    assert "rank" in p.timings and p.timings["rank"] > 0 and "select_matches" not in p.timings

    # the intermediates: exactly the restated stages, and the forest on the kernel's own feature rows of every pair
    assert c.rows.dtype == np.int32 and np.array_equal(c.rows, stages.rows)
    assert c.ratios.dtype == np.uint8 and np.array_equal(c.ratios, stages.ratios)
    assert c.exact.dtype == np.int32 and np.array_equal(c.exact, stages.exact)
    assert c.close.dtype == np.int32 and np.array_equal(c.close, np.where(stages.exact >= 0, -1, stages.close))
    query_table = ds.TitleTable(stages.q_enc, stages.q_len)
    features = ds.construct_features_indexed(query_table, p.truth_table, stages.pair_q, stages.pair_t, ds.SPACE_CODE,
                                             n_truth)
    probabilities = model.predict(features).reshape(n_queries, k)
    assert c.probabilities.dtype == np.float32
    assert np.array_equal(c.probabilities.view(np.uint32), probabilities.view(np.uint32))
    assert np.isfinite(probabilities).all() and (probabilities >= 0).all()

    # the frame: exactly the restated rule on those intermediates
    assert tuple(frame.columns) == prediction.RANKED_COLUMNS
    index = np.arange(n_queries, dtype=np.int64)
    assert _same_frame(frame, _expected_frame(c, 5, n_truth, index, ids))
    assert frame[["test_index", "rank"]].apply(tuple, axis=1).is_monotonic_increasing
    assert (frame.groupby("test_index")["rank"].max() == frame.groupby("test_index").size()).all()
    assert set(frame["stage"].tolist()) == {1, 2, 3}
    assert np.array_equal(frame["title_id"].to_numpy(), ids[frame["match_row"].to_numpy()])
    outside = (stages.exact >= 0) & ~(stages.rows == stages.exact[:, None]).any(axis=1)
    assert outside.any()            # twins of rank >= k: an exact row outside the candidates, ratio 100
    first = frame[frame["rank"] == 1].set_index("test_index")
    assert (first.loc[np.nonzero(outside)[0], "levenshtein_ratio"] == 100).all()

    # n = top_n: every valid candidate, plus the exact row when it lies outside them
    whole = p.ranked_matches(queries, n=k, keep_candidates=True)
    assert _same_frame(whole, _expected_frame(p.candidates, k, n_truth, index, ids))
    listed = whole.groupby("test_index")["match_row"].apply(set)
    for q in range(n_queries):
        rows = set(stages.rows[q].tolist())
        if not outside[q]:
            assert listed[q] == rows, q
        else:
            assert stages.exact[q] in listed[q] and listed[q] - {stages.exact[q]} <= rows and len(listed[q]) == k, q


@pytest.mark.parametrize("k", [10, 100])
def test_rank_one_is_the_answer_of_generate_test_predictions(problem, k):
    truth, ids, queries, model = problem
    p = ds.Prediction(truth, ids, model, top_n=k, transform=False)
    # a threshold between two per-query maxima so that the model stage decides some queries and leaves others
    p.ranked_matches(queries, n=1, keep_candidates=True)
    undecided = (p.candidates.exact < 0) & (p.candidates.close < 0)
    maxima = np.unique(p.candidates.probabilities[undecided].max(axis=1))
    at = int(0.8 * maxima.shape[0])
    p.probability_threshold = float((maxima[at] + maxima[at + 1]) / 2)

    before = p.generate_test_predictions(queries)
    details = p.details.copy()
    timings = set(p.timings)
    ranked = p.ranked_matches(queries, n=3)
    assert p.candidates is None and p.details.equals(details)
    after = p.generate_test_predictions(queries)
    assert before.equals(after) and p.details.equals(details) and set(p.timings) == timings

    answered = details[details["stage"] > 0]
    assert {1, 2, 3} <= set(answered["stage"].tolist()), np.bincount(details["stage"])
    first = ranked[ranked["rank"] == 1].set_index("test_index").loc[answered["test_index"]]
    assert np.array_equal(first["match_row"].to_numpy(), answered["match_row"].to_numpy())
    assert np.array_equal(first["stage"].to_numpy(), answered["stage"].to_numpy())
    assert np.array_equal(first["title_id"].to_numpy(), answered["title_id"].to_numpy())
    assert np.array_equal(first["probability"].to_numpy(), answered["probability"].to_numpy())


def test_the_frame_does_not_depend_on_chunks_preparation_or_order(problem):
    truth, ids, queries, model = problem
    p = ds.Prediction(truth, ids, model, top_n=100, transform=False)
    frame = p.ranked_matches(queries, n=5)
    for chunk in (700, None):
        p.chunk_queries = chunk
        for prepare in ("host", "device"):
            p.prepare_queries = prepare
            assert _same_frame(frame, p.ranked_matches(queries, n=5)), (chunk, prepare)
            assert ("prepare_queries" in p.timings) == (prepare == "device")
    subset = queries[:50]
    p.chunk_queries = None
    whole = p.ranked_matches(subset, n=5)
    assert _same_frame(whole, frame[frame["test_index"] < 50].reset_index(drop=True))
    p.chunk_queries = 1
    assert _same_frame(whole, p.ranked_matches(subset, n=5))
    permutation = np.random.RandomState(4).permutation(50)
    permuted = p.ranked_matches([subset[i] for i in permutation], n=5, test_index=permutation)
    assert _same_frame(whole, permuted)
    p.chunk_queries = None
    reversed_index = p.ranked_matches(subset, n=5, test_index=np.arange(50)[::-1] + 1000)
    assert reversed_index["test_index"].is_monotonic_increasing
    again = whole.copy()
    again["test_index"] = 1049 - again["test_index"]
    again = again.sort_values(["test_index", "rank"], kind="stable").reset_index(drop=True)
    assert _same_frame(again, reversed_index)

    empty = p.ranked_matches([], n=5, keep_candidates=True)
    assert tuple(empty.columns) == prediction.RANKED_COLUMNS and len(empty) == 0
    assert empty.dtypes.tolist() == frame.dtypes.tolist() and p.candidates.rows.shape == (0, 100)
    assert p.timings["rank"] == 0.0
    with pytest.raises(ValueError, match="exceeds the top_n"):
        p.ranked_matches(queries[:3], n=101)
