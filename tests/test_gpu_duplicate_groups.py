"""Prediction.duplicate_groups on the GPU, on the synthetic truth set of the sweep tests (20,000 titles) with duplicates
planted in it: the frame, the counters and the links against the restatement of tests/duplicates_cases.py run on what
ranked_matches keeps of the same truth titles (the parent's own scores), the planted groups, and the variants that must
not change the frame."""
import numpy as np
import pandas as pd
import pytest

import doppel_speller_amd as ds
import duplicates_cases as dc
from doppel_speller_amd import prediction, synth

pytestmark = pytest.mark.gpu

TOP_N = 10
N_TRUTH = 20000
LETTERS = "abcdefghijklmnopqrstuvwxyz"


def _substitute(title, rng, avoid=()):
    """(title with one letter replaced by another letter, the position): the title stays a transformed title."""
    positions = [i for i, c in enumerate(title) if c in LETTERS and i not in avoid]
    at = positions[rng.randint(len(positions))]
    other = LETTERS[(LETTERS.index(title[at]) + 1 + rng.randint(25)) % 26]
    return title[:at] + other + title[at + 1:], at


def plant(truth):
    """Overwrites 800 rows of `truth` out of 1,200 chosen ones: 300 verbatim copies (of 300 chosen sources), 300 copies
    with one character substituted (of titles of 20 characters at least, ratio (2L - 2) / 2L > 94), and 100 chains a -> a'
    -> a'' of two successive substitutions (of 100 chosen heads).  -> (copies, substitutions, chains) as row tuples."""
    rng = np.random.RandomState(77)
    chosen = rng.permutation(len(truth))[:1200]
    targets, copy_sources, heads = chosen[:800], chosen[800:1100], chosen[1100:]
    free = np.setdiff1d(np.arange(len(truth)), chosen)
    long_enough = [int(r) for r in free if len(truth[r]) >= 20]
    copies = [(int(s), int(t)) for s, t in zip(copy_sources, targets[:300])]
    for source, target in copies:
        truth[target] = truth[source]
    substitutions = [(long_enough[i], int(t)) for i, t in zip(rng.permutation(len(long_enough))[:300], targets[300:600])]
    for source, target in substitutions:
        truth[target] = _substitute(truth[source], rng)[0]
    chains = []
    for head, first, second in zip(heads, targets[600:700], targets[700:800]):
        truth[first], at = _substitute(truth[head], rng)
        truth[second] = _substitute(truth[first], rng, avoid=(at,))[0]
        chains.append((int(head), int(first), int(second)))
    # what the planted set holds, checked where it is made
    differ = lambda a, b: len(a) == len(b) and sum(x != y for x, y in zip(a, b))
    assert sum(truth[s] == truth[t] for s, t in copies) >= 20
    assert sum(differ(truth[s], truth[t]) == 1 and len(truth[s]) >= 20 for s, t in substitutions) >= 20
    assert sum(differ(truth[a], truth[b]) == 1 and differ(truth[b], truth[c]) == 1 and differ(truth[a], truth[c]) == 2
               for a, b, c in chains) >= 10
    return copies, substitutions, chains


@pytest.fixture(scope="module")
def problem():
    w = synth.make_workload(N_TRUTH, 400)
    truth = synth._to_strings(w.t_flat, w.t_off)
    planted = plant(truth)
    forest = synth.make_forest(n_trees=100)
    model = ds.ForestModel(forest["feature"], forest["threshold"], forest["yes"], forest["no"], forest["missing"],
                           forest["tree_offsets"], forest["n_features"], forest["base_margin"])
    p = ds.Prediction(truth, w.title_id, model, top_n=TOP_N, transform=False)
    return p, truth, np.asarray(w.title_id, dtype=np.int64), planted


def _scores(p, truth, t):
    """The parent's own scores of the truth titles as queries at Levenshtein threshold t (the close stage's ratio depends
    on it): Candidates of ranked_matches."""
    held = p.levenshtein_threshold
    p.levenshtein_threshold = t
    try:
        p.ranked_matches(truth, n=1, keep_candidates=True)
    finally:
        p.levenshtein_threshold = held
    return p.candidates


def _expected(candidates, ids, t, u, model_links=True):
    probabilities = candidates.probabilities if model_links else None
    edges, reasons, counts = dc.links_of(candidates.rows, candidates.ratios, probabilities, candidates.exact, 0, N_TRUTH, t, u)
    labels, sizes = dc.components(N_TRUTH, edges)
    # the links restated column by column, not by the code under test
    links = pd.DataFrame(dc.link_columns(candidates.rows, candidates.ratios, probabilities, candidates.exact, 0, N_TRUTH,
                                         t, u, ids), columns=list(prediction.LINK_COLUMNS))
    assert np.array_equal(links[["row", "match_row"]].to_numpy(), edges)
    return prediction.duplicate_frame(labels, sizes, ids), dict(zip(("exact", "close", "model"), counts.tolist())), links


def _same_frame(a, b):
    return list(a.columns) == list(b.columns) and a.dtypes.tolist() == b.dtypes.tolist() and all(
        np.array_equal(a[c].to_numpy(), b[c].to_numpy(), equal_nan=a[c].dtype.kind == "f") for c in a.columns)


@pytest.fixture(scope="module")
def grouped(problem):
    """The default call at (94, 0.9) with its links, next to the parent's scores at 94."""
    p, truth, ids, _ = problem
    candidates = _scores(p, truth, 94)
    details = p.details
    frame = p.duplicate_groups(return_links=True)
    assert p.candidates is candidates and p.details is details           # left alone
    return frame, dict(p.link_counts), p.links, dict(p.timings), candidates


def test_the_frame_counts_and_links_are_the_restatement_on_the_parents_scores(problem, grouped):
    p, truth, ids, _ = problem
    frame, counts, links, timings, candidates = grouped
    expected_frame, expected_counts, expected_links = _expected(candidates, ids, 94, 0.9)
    assert _same_frame(frame, expected_frame)
    assert counts == expected_counts and counts["exact"] > 0 and counts["close"] > 0
    assert _same_frame(links, expected_links)
    assert tuple(frame.columns) == prediction.DUPLICATE_COLUMNS and tuple(links.columns) == prediction.LINK_COLUMNS
    assert len(links) == sum(counts.values()) and {1, 2} <= set(links["stage"].tolist())
    assert set(timings) == {"prepare_queries", "top_k", "close_matches", "exact_matches", "features", "model", "links",
                            "finish", "copy_back", "host_prepare"}
    assert all(timings[name] > 0 for name in ("top_k", "close_matches", "features", "model", "links", "finish"))
    # the shape of the answer: sorted by the group's lowest row, then by row; group_id is that row's title id
    lowest = frame.groupby("group_id", sort=False)["row"].transform("min").to_numpy()
    assert np.array_equal(ids[lowest], frame["group_id"].to_numpy())
    order = np.lexsort((frame["row"].to_numpy(), lowest))
    assert np.array_equal(order, np.arange(len(frame)))
    assert np.array_equal(frame.groupby("group_id", sort=False)["row"].transform("size").to_numpy(),
                          frame["group_size"].to_numpy()) and frame["group_size"].min() >= 2
    assert np.array_equal(ids[frame["row"].to_numpy()], frame["title_id"].to_numpy())


@pytest.fixture(scope="module")
def other_cell(problem):
    """Levenshtein threshold 85 and a probability threshold the model's own scores suggest: the 50th highest distinct
    probability among the slots that hold another row and are not close, so that the model alone links some pairs (at
    0.9 the synthetic forest links none).  -> (the parent's scores at 85, u)."""
    p, truth, _, _ = problem
    candidates = _scores(p, truth, 85)
    others = (candidates.rows != np.arange(N_TRUTH)[:, None]) & (candidates.ratios <= 85)
    values = np.unique(candidates.probabilities[others])
    assert values.shape[0] >= 100
    return candidates, float(values[-50])


def test_another_cell(problem, other_cell):
    p, truth, ids, _ = problem
    candidates, u = other_cell
    frame = p.duplicate_groups(85, u, return_links=True)
    expected_frame, expected_counts, expected_links = _expected(candidates, ids, 85, u)
    assert expected_counts["model"] > 0                                   # by the restatement: the cell has model links
    assert _same_frame(frame, expected_frame) and p.link_counts == expected_counts and _same_frame(p.links, expected_links)
    assert set(p.links["stage"].tolist()) == {1, 2, 3}
    # the instance's own thresholds are what None takes
    p.levenshtein_threshold, p.probability_threshold = 85, u
    try:
        assert _same_frame(frame, p.duplicate_groups())
        assert p.links is None and p.link_counts == expected_counts
    finally:
        p.levenshtein_threshold, p.probability_threshold = 94, 0.9


def test_the_planted_duplicates(problem, grouped):
    _, truth, _, (copies, substitutions, chains) = problem
    frame, _, links, _, _ = grouped
    group = dict(zip(frame["row"].tolist(), frame["group_id"].tolist()))
    for source, target in copies:
        assert source in group and group[source] == group.get(target), (source, target)
    # a substitution in a title of 20 characters is above 94: linked wherever the candidate stage shows the source
    found = sum(group.get(s, -1) == group.get(t, -2) for s, t in substitutions)
    assert found >= 20
    # transitivity: a group with two rows that no link joins directly
    linked = set(zip(links["row"].tolist(), links["match_row"].tolist()))
    apart = 0
    for a, b, c in chains:
        if group.get(a, -1) == group.get(b, -2) == group.get(c, -3) and (a, c) not in linked and (c, a) not in linked:
            apart += 1
    assert apart >= 1


def test_without_the_model(problem, grouped, other_cell):
    p, truth, ids, _ = problem
    _, counts, _, _, candidates = grouped
    alone = p.duplicate_groups(model_links=False, return_links=True)
    expected_frame, expected_counts, expected_links = _expected(candidates, ids, 94, 0.9, model_links=False)
    assert _same_frame(alone, expected_frame) and p.link_counts == expected_counts and _same_frame(p.links, expected_links)
    assert p.link_counts == dict(counts, model=0) and p.links["probability"].isna().all()
    assert p.timings["features"] == 0 and p.timings["model"] == 0 and p.timings["links"] > 0
    # in the cell where the model links pairs: the groups without it refine those with it (rows it joins are joined there)
    candidates, u = other_cell
    alone = p.duplicate_groups(85, u, model_links=False)
    assert _same_frame(alone, _expected(candidates, ids, 85, u, model_links=False)[0])
    assert p.link_counts["model"] == 0 and p.timings["features"] == 0
    frame = p.duplicate_groups(85, u)
    coarse = dict(zip(frame["row"].tolist(), frame["group_id"].tolist()))
    fine = alone.groupby("group_id")["row"].apply(list)
    assert all(len({coarse.get(row, -1 - row) for row in rows}) == 1 for rows in fine)
    assert len(alone) <= len(frame)


def test_the_frame_does_not_depend_on_the_chunks_or_the_call(problem, grouped):
    p, _, _, _ = problem
    frame, counts, links, _, _ = grouped
    try:
        for chunk in (20000, 7001, 1_000_000):
            p.chunk_queries = chunk
            again = p.duplicate_groups(return_links=chunk == 7001)
            assert _same_frame(frame, again) and p.link_counts == counts, chunk
            if chunk == 7001:
                assert _same_frame(links, p.links)
    finally:
        p.chunk_queries = None
    assert _same_frame(frame, p.duplicate_groups()) and p.links is None


def test_validation_errors(problem):
    p = problem[0]
    counts = p.link_counts
    for lev, prob, message in ((101, None, r"\[0, 100\]"), (True, None, "integer"), (94.0, None, "integer"),
                               (None, float("nan"), "finite"), (None, "0.9", "finite number")):
        with pytest.raises(ValueError, match=message):
            p.duplicate_groups(lev, prob)
    assert p.link_counts is counts


def test_a_truth_set_without_duplicates_gives_an_empty_frame():
    w = synth.make_workload(3000, 10)
    truth = sorted(set(synth._to_strings(w.t_flat, w.t_off)))
    forest = synth.make_forest(n_trees=20)
    model = ds.ForestModel(forest["feature"], forest["threshold"], forest["yes"], forest["no"], forest["missing"],
                           forest["tree_offsets"], forest["n_features"], forest["base_margin"])
    p = ds.Prediction(truth, np.arange(len(truth)), model, top_n=5, transform=False, levenshtein_threshold=100,
                      probability_threshold=1.0)
    frame = p.duplicate_groups(return_links=True)
    assert len(frame) == 0 and tuple(frame.columns) == prediction.DUPLICATE_COLUMNS
    assert frame.dtypes.tolist() == [np.int64] * 4
    assert p.link_counts == {"exact": 0, "close": 0, "model": 0}
    assert len(p.links) == 0 and tuple(p.links.columns) == prediction.LINK_COLUMNS
