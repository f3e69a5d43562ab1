"""Prediction.one_to_one_matches on the GPU, on the problem of tests/test_gpu_ranked_matches.py (rebuilt here) with 300 more
queries made to contend: for 100 truth titles one verbatim copy and two copies with one character changed.  The frame, the
`assignment` and the counts against the restatement of tests/assignment_cases.py applied to ranked_matches(titles, n) of the
same instance, bit for bit; then what the matching must hold whatever the restatement says, and the variants that must not
change it."""
import numpy as np
import pytest

import assignment_cases as ac
import doppel_speller_amd as ds
from doppel_speller_amd import prediction, synth

pytestmark = pytest.mark.gpu

N_BASE, N_PLANTED = 2000, 100


@pytest.fixture(scope="module")
def problem():
    """20,040 truth titles (40 of them duplicates under new ids) and 2,300 queries: the 2,000 of the ranked-matches problem,
    then per planted truth row a verbatim copy (2000 + 3 i) and two copies with one character changed (+ 1, + 2)."""
    w = synth.make_workload(20000, N_BASE)
    truth = synth._to_strings(w.t_flat, w.t_off)
    ids = list(w.title_id)
    rng = np.random.RandomState(21)
    duplicated = rng.randint(0, 20000, 40)
    truth += [truth[i] for i in duplicated]
    ids += list(range(20000, 20040))
    queries = synth._to_strings(w.q_flat, w.q_off)
    verbatim = rng.permutation(N_BASE)[:200]
    sources = np.concatenate((duplicated[:20], rng.randint(0, len(truth), 180)))
    for q, t in zip(verbatim, sources):
        queries[q] = truth[t]
    # rows whose title no other truth row and no query so far holds, long enough for one changed character to stay close
    held = {}
    for title in truth:
        held[title] = held.get(title, 0) + 1
    taken = set(queries)
    free = [t for t, title in enumerate(truth) if held[title] == 1 and title not in taken and len(title) >= 30]
    planted = np.array(free)[rng.permutation(len(free))[:N_PLANTED]]
    assert planted.shape[0] == N_PLANTED
    for t in planted:
        title = truth[t]
        queries.append(title)
        for _ in range(2):
            while True:
                at = int(rng.randint(0, len(title)))
                letter = "abcdefghijklmnopqrstuvwxyz"[rng.randint(0, 26)]
                changed = title[:at] + letter + title[at + 1:]
                if title[at] != " " and letter != title[at] and changed not in held and changed not in taken:
                    break
            taken.add(changed)
            queries.append(changed)
    forest = synth.make_forest(n_trees=100)
    model = ds.ForestModel(forest["feature"], forest["threshold"], forest["yes"], forest["no"], forest["missing"],
                           forest["tree_offsets"], forest["n_features"], forest["base_margin"])
    return truth, np.array(ids, dtype=np.int64), queries, model, planted


def slots_of(frame, count, n):
    """The [Q, n] slots of the rank stage back from ranked_matches' long frame (test_index = the title's number)."""
    rows, probabilities = np.full((count, n), -1, np.int32), np.full((count, n), np.nan, np.float32)
    ratios, stages = np.zeros((count, n), np.uint8), np.zeros((count, n), np.int8)
    q, s = frame["test_index"].to_numpy(), frame["rank"].to_numpy() - 1
    rows[q, s], probabilities[q, s] = frame["match_row"].to_numpy(), frame["probability"].to_numpy()
    ratios[q, s], stages[q, s] = frame["levenshtein_ratio"].to_numpy(), frame["stage"].to_numpy()
    return rows, probabilities, ratios, stages


def same_frame(a, b):
    return list(a.columns) == list(b.columns) and a.dtypes.tolist() == b.dtypes.tolist() and all(
        np.array_equal(np.ascontiguousarray(a[c].to_numpy()).view(np.uint8),
                       np.ascontiguousarray(b[c].to_numpy()).view(np.uint8)) for c in a.columns)


@pytest.fixture(scope="module")
def solved(problem):
    """One instance, the threshold put where the model has a say (the synthetic forest puts no pair above 0.9: the median
    of the model slots' probabilities instead), one call at n = 5 and the restatement on the ranked slots of the same call."""
    truth, ids, queries, model, planted = problem
    p = ds.Prediction(truth, ids, model, top_n=100, transform=False)
    ranked = p.ranked_matches(queries, n=5)
    p.probability_threshold = float(np.median(ranked.loc[ranked["stage"] == 3, "probability"].to_numpy()))
    frame = p.one_to_one_matches(queries, n=5)
    slots = slots_of(ranked, len(queries), 5)
    keys = ac.edge_keys(*slots, 0, len(truth), np.float32(p.probability_threshold))
    want = ac.deferred_acceptance(slots[0], keys, len(truth))
    return p, frame, p.assignment.copy(), dict(p.assignment_counts), dict(p.timings), slots, keys, want


def test_the_answer_is_the_restated_matching_of_the_ranked_slots(problem, solved):
    truth, ids, queries, model, planted = problem
    p, frame, assignment, counts, timings, slots, keys, want = solved
    index = np.arange(len(queries), dtype=np.int64)
    assert same_frame(frame, prediction.finalize_output(index, want.match_row, ids))
    assert same_frame(assignment, prediction.assignment_frame(index, want.match_row, want.match_slot, want.first_row, *slots,
                                                              ids))
    assert list(counts) == list(prediction.ASSIGNMENT_COUNTS)
    assert [counts[name] for name in prediction.ASSIGNMENT_COUNTS[:4]] == want.counts.tolist()
    assert counts["matched"] <= counts["proposals"] <= counts["edges"] and 1 <= counts["rounds"] <= counts["proposals"] + 1
    assert ac.is_stable(slots[0], keys, len(truth), assignment["match_row"].to_numpy(), assignment["rank"].to_numpy() - 1)
    assert {1, 2, 3} <= set(assignment["stage"].tolist()) and (keys >> np.uint64(62) == 1).sum() > 1000
    for name in ("assign_edges", "assign", "rank", "top_k", "model"):
        assert timings[name] > 0, name
    assert "select_matches" not in timings
    assert list(frame.columns) == ["title_id", "test_index"] and frame["test_index"].tolist() == index.tolist()


def test_no_truth_row_twice_and_the_planted_contenders(problem, solved):
    truth, ids, queries, model, planted = problem
    p, frame, assignment, counts, timings, slots, keys, want = solved
    matched = assignment[assignment["match_row"] >= 0]
    assert not matched["match_row"].duplicated().any() and not frame.loc[frame["title_id"] >= 0, "title_id"].duplicated().any()
    copies = assignment.iloc[N_BASE::3]
    assert np.array_equal(copies["match_row"].to_numpy(), planted) and (copies["stage"] == 1).all()
    assert (copies["probability"] == 1.0).all() and (copies["rank"] == 1).all() and not copies["displaced"].any()
    near = assignment.iloc[[N_BASE + 3 * i + j for i in range(N_PLANTED) for j in (1, 2)]]
    assert not np.isin(near["match_row"].to_numpy(), planted).any()
    assert (near["first_choice_row"].to_numpy() == np.repeat(planted, 2)).mean() > 0.9 and near["displaced"].sum() > 150
    assert counts["displaced"] > 0 and counts["displaced"] == int(assignment["displaced"].sum())
    assert counts["displaced_unmatched"] == int((assignment["displaced"] & (assignment["match_row"] < 0)).sum())


def test_a_title_nobody_contends_with_gets_its_first_edge(solved):
    p, frame, assignment, counts, timings, slots, keys, want = solved
    edge = keys != 0
    first = assignment["first_choice_row"].to_numpy()
    claims = np.bincount(slots[0][edge], minlength=len(p.truth_titles))          # edges into every row, from any slot
    alone = (first >= 0) & (claims[np.maximum(first, 0)] == 1)
    assert alone.sum() > 500 and (~alone & (first >= 0)).sum() > 200
    assert np.array_equal(assignment["match_row"].to_numpy()[alone], first[alone])
    assert (assignment["rank"].to_numpy()[alone] >= 1).all() and not assignment["displaced"].to_numpy()[alone].any()


def test_the_answer_does_not_depend_on_chunks_preparation_or_index_build(problem, solved):
    truth, ids, queries, model, planted = problem
    p, frame, assignment, counts, timings, slots, keys, want = solved
    try:
        for chunk, prepare in ((137, "device"), (1000, "host"), (None, "host")):
            p.chunk_queries, p.prepare_queries = chunk, prepare
            assert same_frame(frame, p.one_to_one_matches(queries, n=5)), (chunk, prepare)
            assert same_frame(assignment, p.assignment), (chunk, prepare)
            assert [p.assignment_counts[name] for name in prediction.ASSIGNMENT_COUNTS[:4]] == want.counts.tolist()
            assert ("prepare_queries" in p.timings) == (prepare == "device")
    finally:
        p.chunk_queries, p.prepare_queries = None, "device"
    other = ds.Prediction(truth, ids, model, top_n=100, transform=False, build_index="device", chunk_queries=1000,
                          probability_threshold=p.probability_threshold)
    assert same_frame(frame, other.one_to_one_matches(queries, n=5)) and same_frame(assignment, other.assignment)
    # the threshold as an argument, and another test index: the same matching under other names
    other.probability_threshold = 0.9
    index = np.arange(len(queries))[::-1] + 500
    renamed = other.one_to_one_matches(queries, n=5, test_index=index, probability_threshold=p.probability_threshold)
    assert renamed["test_index"].is_monotonic_increasing
    assert np.array_equal(renamed["title_id"].to_numpy()[::-1], frame["title_id"].to_numpy())
    assert np.array_equal(other.assignment["test_index"].to_numpy(), index)
    assert np.array_equal(other.assignment["match_row"].to_numpy(), assignment["match_row"].to_numpy())


def test_one_slot_per_title_no_title_and_what_a_call_leaves_alone(problem, solved):
    truth, ids, queries, model, planted = problem
    p, frame, assignment, counts, timings, slots, keys, want = solved
    before = p.generate_test_predictions(queries[:300])
    details = p.details.copy()
    kept = (p.candidates, p.links, p.contributions)
    subset = queries[N_BASE - 100:N_BASE + 200]
    ranked = p.ranked_matches(subset, n=1)
    one = p.one_to_one_matches(subset, n=1)
    assert p.details.equals(details) and (p.candidates, p.links, p.contributions) == kept
    own = slots_of(ranked, len(subset), 1)
    own_keys = ac.edge_keys(*own, 0, len(truth), np.float32(p.probability_threshold))
    expected = ac.deferred_acceptance(own[0], own_keys, len(truth))
    assert np.array_equal(p.assignment["match_row"].to_numpy(), expected.match_row)
    assert set(p.assignment["rank"].tolist()) == {0, 1}
    assert p.assignment_counts["displaced"] == p.assignment_counts["displaced_unmatched"] > 0
    assert same_frame(one, prediction.finalize_output(np.arange(len(subset)), expected.match_row, ids))
    assert same_frame(before, p.generate_test_predictions(queries[:300]))

    empty = p.one_to_one_matches([], n=5)
    assert list(empty.columns) == ["title_id", "test_index"] and len(empty) == 0 and len(p.assignment) == 0
    assert tuple(p.assignment.columns) == prediction.ASSIGNMENT_COLUMNS
    assert p.assignment.dtypes.tolist() == assignment.dtypes.tolist()
    assert p.assignment_counts == dict.fromkeys(prediction.ASSIGNMENT_COUNTS, 0) and p.timings["assign"] == 0.0
    with pytest.raises(ValueError, match="exceeds the top_n"):
        p.one_to_one_matches(queries[:3], n=101)
    with pytest.raises(ValueError, match="probability_threshold"):
        p.one_to_one_matches(queries[:3], probability_threshold=float("nan"))


def test_the_memory_is_checked_before_anything_is_allocated(problem, solved, monkeypatch):
    truth, ids, queries, model, planted = problem
    p = solved[0]
    import ctypes
    from doppel_speller_amd import _lib

    def free_bytes():
        free, total = ctypes.c_int64(0), ctypes.c_int64(0)
        _lib.check(_lib.lib().ds_device_memory(0, ctypes.byref(free), ctypes.byref(total)), "ds_device_memory")
        return free.value

    before = free_bytes()
    monkeypatch.setattr(prediction, "ASSIGN_RESERVE_BYTES", 1 << 50)
    with pytest.raises(ds.DoppelError, match="bytes of HBM"):
        p.one_to_one_matches(queries[:100], n=5)
    assert free_bytes() >= before
