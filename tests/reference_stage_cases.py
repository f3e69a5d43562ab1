"""The fixtures tests/golden/make_golden_predict.py captured from the reference's own train.py and predict.py bodies
(train_objective.npz, predict_stages.npz, predict_end_to_end.npz), loaded once, and what the CPU and the GPU test of them share: the captured
answer of every stage per title, in title ids, and the lookup forests that plant a margin per row or per (title, candidate)
pair.  A plain module like sweep_cases.py: no fixtures, no GPU.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load(name):
    with np.load(os.path.join(GOLDEN, name), allow_pickle=False) as archive:
        return {key: archive[key] for key in archive.files}


def _text(values):
    return [v.decode("utf-8") for v in values.tolist()]


OBJECTIVE = _load("train_objective.npz")
STAGES = _load("predict_stages.npz")
THRESHOLDS = [float(t) for t in STAGES["thresholds"]]              # the reference's own 0.9 first
LEVENSHTEIN_THRESHOLD = int(STAGES["levenshtein_threshold"])
NOT_FOUND = int(STAGES["not_found"])
TOP_N = int(STAGES["top_n"])

PAIR_X, PAIR_Y = _text(STAGES["pair_x"]), _text(STAGES["pair_y"])
TRUTH_TITLES, TITLES, NAMES = _text(STAGES["truth_titles"]), _text(STAGES["titles"]), _text(STAGES["names"])
TRUTH_IDS = STAGES["truth_ids"].astype(np.int64)
ROWS = STAGES["candidate_rows"].astype(np.int32)                   # [titles, TOP_N] truth rows of the planted candidates
PROBABILITIES = STAGES["probabilities"].astype(np.float32)         # [titles, TOP_N] planted
RATIOS = STAGES["candidate_ratios"].astype(np.int64)               # [titles, TOP_N] _get_levenshtein_ratio of every pair
N_TITLES, N_TRUTH = len(TITLES), len(TRUTH_TITLES)


def ids_of(rows):
    """The title id of every truth row of `rows`, NOT_FOUND where the row is negative."""
    rows = np.asarray(rows).astype(np.int64)
    return np.where(rows >= 0, TRUTH_IDS[np.maximum(rows, 0)], NOT_FOUND)


def stage_ids(i):
    """(exact, close, model) int64[titles]: the title id the reference's stage saved for every title at THRESHOLDS[i],
    NOT_FOUND where it saved none.  The saved frame holds the stages' blocks in their order (predict.py:84-93)."""
    index, ids = STAGES[f"saved_index_{i}"], STAGES[f"saved_id_{i}"]
    a, b, c = STAGES["after_exact"].shape[0], STAGES["after_close"].shape[0], STAGES[f"after_model_{i}"].shape[0]
    assert c == index.shape[0] and np.array_equal(index, STAGES[f"after_model_{i}"])
    assert np.array_equal(index[:a], STAGES["after_exact"]) and np.array_equal(index[:b], STAGES["after_close"])
    out = []
    for first, last in ((0, a), (a, b), (b, c)):
        stage = np.full(N_TITLES, NOT_FOUND, dtype=np.int64)
        stage[index[first:last]] = ids[first:last]
        out.append(stage)
    return tuple(out)


def final_ids(i):
    """int64[titles]: the final table's title id per test index at THRESHOLDS[i] (the table is sorted by test index)."""
    assert np.array_equal(STAGES[f"final_index_{i}"], np.arange(N_TITLES))
    return STAGES[f"final_id_{i}"].astype(np.int64)


def actual_rows():
    """int32[titles]: the truth row of every planted actual id, -1 for none, and a row beyond the truth set for the id
    no truth row has (a prediction never equals it)."""
    row_of = {int(title_id): row for row, title_id in enumerate(TRUTH_IDS)}
    return np.array([-1 if a == NOT_FOUND else row_of.get(int(a), N_TRUTH + 5) for a in STAGES["actual_ids"]],
                    dtype=np.int32)


def remaining_probabilities(pair_q):
    """The planted probability of every pair of a remaining pair list (TOP_N consecutive pairs per title)."""
    pair_q = np.asarray(pair_q).astype(np.int64)
    return PROBABILITIES[pair_q, np.arange(pair_q.shape[0]) % TOP_N]


# ---- the stages behind the reference's own MatchMaker (predict_end_to_end.npz) ------------------------------------------

END_TO_END = _load("predict_end_to_end.npz")
E2E_TRUTH_TITLES, E2E_TITLES, E2E_NAMES = (_text(END_TO_END[name]) for name in ("truth_titles", "titles", "names"))
E2E_TRUTH_IDS = END_TO_END["truth_ids"].astype(np.int64)


def e2e_stage_ids():
    """(exact, close, model) int64[titles] as stage_ids, for the titles of predict_end_to_end.npz."""
    e = END_TO_END
    index, ids = e["saved_index"], e["saved_id"]
    a, b, c = e["after_exact"].shape[0], e["after_close"].shape[0], e["after_model"].shape[0]
    assert c == index.shape[0] and np.array_equal(index, e["after_model"])
    out = []
    for first, last in ((0, a), (a, b), (b, c)):
        stage = np.full(len(E2E_TITLES), NOT_FOUND, dtype=np.int64)
        stage[index[first:last]] = ids[first:last]
        out.append(stage)
    return tuple(out)


def _tree(nodes):
    feature, threshold, yes, no = (np.array([n[i] for n in nodes], dtype=dtype)
                                   for i, dtype in enumerate((np.int32, np.float32, np.int32, np.int32)))
    return dict(feature=feature, threshold=threshold, yes=yes, no=no, missing=no.copy(),
                tree_offsets=np.array([0, len(nodes)], np.int64))


def margin_lookup_forest(margins):
    """One tree that gives row i (feature 0 = i + 0.5) the margin margins[i]: a chain of splits on feature 0."""
    nodes = []
    for i, margin in enumerate(margins[:-1]):
        nodes += [[0, i + 1, 2 * i + 1, 2 * i + 2], [-1, margin, 0, 0]]
    return _tree(nodes + [[-1, margins[-1], 0, 0]])


def pair_lookup_forest(title_lengths, truth_lengths, margins, default):
    """One tree that tells a (title, candidate) pair by feature 0, the title's characters, and feature 1, the truth title's
    (construct_features' first two columns): a chain over the title lengths, under each a chain over the lengths of that
    title's candidates [titles, k] with the margin planted for it [titles, k]; any other pair gets `default`.  The title
    lengths are all different; candidates of one title with one length hold one margin."""
    nodes = []

    def chain(feature, items):
        at = len(nodes)
        nodes.append(None)
        if not items:
            nodes[at] = [-1, default, 0, 0]
            return at
        (key, below), rest = items[0], items[1:]
        yes = below()
        nodes[at] = [feature, key + 0.5, yes, chain(feature, rest)]
        return at

    def leaf(margin):
        nodes.append([-1, margin, 0, 0])
        return len(nodes) - 1

    assert len(set(title_lengths)) == len(title_lengths)
    titles = []
    for q in np.argsort(title_lengths):
        held = {}
        for length, margin in zip(truth_lengths[q], margins[q]):
            assert held.setdefault(int(length), float(margin)) == float(margin)
        under = [(length, (lambda m=m: leaf(m))) for length, m in sorted(held.items())]
        titles.append((int(title_lengths[q]), (lambda under=under: chain(1, under))))
    assert chain(0, titles) == 0
    return _tree(nodes)
