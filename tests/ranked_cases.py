"""The ranking rule of ds_rank_matches_device (include/doppel_amd.h, DESIGN.md section 8 "Ranked matches") restated twice,
and the groups of candidates the tests rank.

    rank_matches          NumPy, whole arrays at once: what the kernel and Prediction.ranked_matches are compared against
    rank_matches_python   a query at a time with sorted(): what rank_matches is compared against

Per query: the head (the exact row, else the best close row) takes slot 0 with probability 1.0 and the ratio of the first
candidate that equals it (absent from the candidates: 100 for an exact head, 0 for a close one); the rest (candidates
with a row inside the truth table that is not the head) follows at stage 3 by the float32 bits of the probability
descending, then by the position ascending; the list is cut to n slots, an unfilled slot is (-1, NaN, 0, 0)."""
import numpy as np

EMPTY_PROBABILITY = np.array([0x7fc00000], dtype=np.uint32).view(np.float32)[0]


def heads(exact, best, n_queries):
    """(head row or -1, stage 1 / 2 / 0) per query; exact / best: int arrays or None ("no such stage")."""
    exact = np.full(n_queries, -1, np.int64) if exact is None else np.asarray(exact, dtype=np.int64)
    best = np.full(n_queries, -1, np.int64) if best is None else np.asarray(best, dtype=np.int64)
    head = np.where(exact >= 0, exact, np.where(best >= 0, best, -1))
    stage = np.where(exact >= 0, 1, np.where(best >= 0, 2, 0))
    return head, stage


def rank_matches(rows, probabilities, ratios, exact, best, n, n_truth):
    """-> (row int32[Q, n], probability float32[Q, n], ratio uint8[Q, n], stage int8[Q, n])"""
    rows = np.asarray(rows, dtype=np.int64)
    probabilities = np.ascontiguousarray(probabilities, dtype=np.float32)
    ratios = np.asarray(ratios, dtype=np.uint8)
    n_queries, k = rows.shape
    head, head_stage = heads(exact, best, n_queries)
    lead = (head >= 0).astype(np.int64)
    is_head = (rows == head[:, None]) & (head >= 0)[:, None]
    rest = (rows >= 0) & (rows < n_truth) & ~is_head
    # descending (bits, -position) = ascending (~bits, position), the skipped candidates last
    bits = probabilities.view(np.uint32).astype(np.uint64)
    position = np.broadcast_to(np.arange(k, dtype=np.uint64), rows.shape)
    sort_key = np.where(rest, ((np.uint64(0xffffffff) - bits) << np.uint64(32)) | position, ~np.uint64(0))
    order = np.argsort(sort_key, axis=1, kind="stable")
    n_rest = rest.sum(axis=1)

    out_row = np.full((n_queries, n), -1, dtype=np.int32)
    out_probability = np.full((n_queries, n), EMPTY_PROBABILITY, dtype=np.float32)
    out_ratio = np.zeros((n_queries, n), dtype=np.uint8)
    out_stage = np.zeros((n_queries, n), dtype=np.int8)
    slot = np.arange(n, dtype=np.int64)[None, :]
    source = slot - lead[:, None]                       # which of the ordered rest fills the slot
    filled = (source >= 0) & (source < n_rest[:, None])
    take = np.take_along_axis(order, np.clip(source, 0, k - 1), axis=1)
    out_row[filled] = np.take_along_axis(rows, take, axis=1)[filled]
    out_probability[filled] = np.take_along_axis(probabilities, take, axis=1)[filled]
    out_ratio[filled] = np.take_along_axis(ratios, take, axis=1)[filled]
    out_stage[filled] = 3
    with_head = head >= 0
    first = np.argmax(is_head, axis=1)
    present = is_head.any(axis=1)
    head_ratio = np.where(present, ratios[np.arange(n_queries), first], np.where(head_stage == 1, 100, 0))
    out_row[with_head, 0] = head[with_head]
    out_probability[with_head, 0] = 1.0
    out_ratio[with_head, 0] = head_ratio[with_head]
    out_stage[with_head, 0] = head_stage[with_head]
    return out_row, out_probability, out_ratio, out_stage


def rank_matches_python(rows, probabilities, ratios, exact, best, n, n_truth):
    """The same lists, one query at a time: [[(row, probability bits, ratio, stage)] * n] * Q."""
    rows = np.asarray(rows)
    bits = np.ascontiguousarray(probabilities, dtype=np.float32).view(np.uint32)
    out = []
    for q in range(rows.shape[0]):
        e = -1 if exact is None else int(exact[q])
        b = -1 if best is None else int(best[q])
        head, stage = (e, 1) if e >= 0 else ((b, 2) if b >= 0 else (-1, 0))
        ranked = []
        if head >= 0:
            same = [j for j in range(rows.shape[1]) if int(rows[q, j]) == head]
            ratio = int(ratios[q, same[0]]) if same else (100 if stage == 1 else 0)
            ranked.append((head, 0x3f800000, ratio, stage))
        rest = [j for j in range(rows.shape[1]) if 0 <= int(rows[q, j]) < n_truth and int(rows[q, j]) != head]
        for j in sorted(rest, key=lambda j: (-int(bits[q, j]), j)):
            ranked.append((int(rows[q, j]), int(bits[q, j]), int(ratios[q, j]), 3))
        ranked = ranked[:n] + [(-1, 0x7fc00000, 0, 0)] * max(0, n - len(ranked))
        out.append(ranked)
    return out


def as_lists(ranked):
    """rank_matches' arrays in the form of rank_matches_python."""
    row, probability, ratio, stage = ranked
    bits = np.ascontiguousarray(probability).view(np.uint32)
    return [[(int(row[q, s]), int(bits[q, s]), int(ratio[q, s]), int(stage[q, s])) for s in range(row.shape[1])]
            for q in range(row.shape[0])]


def same_ranking(a, b):
    """Bit for bit: the probabilities compared as their uint32 bits (the empty slots hold a NaN)."""
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
               and x.dtype == y.dtype and x.shape == y.shape for x, y in zip(a, b))


def make_groups(n_queries, k, n_truth, seed, ties="some"):
    """Candidate groups with every situation of the rule in turn (query q is of kind q % 8):
         0  no head                          4  close head among the candidates
         1  exact head among the candidates  5  no head, rows of -1 and rows >= n_truth among the candidates
         2  exact head outside them          6  exact head twice among the candidates, and invalid rows
         3  exact and close head, both among the candidates (the exact one wins, the close one is ranked as the rest)
         7  every candidate invalid, close head outside the candidates
    ties: "none" distinct probabilities, "some" 2-way and larger ties, "all" one probability per query, "k" one
    probability for the whole array.  -> rows int32[Q, k], probabilities float32[Q, k], ratios uint8[Q, k], exact
    int32[Q], best int32[Q] (best as the exact stage leaves it, the exact row where there is one, but for kind 3)."""
    assert n_truth >= 2 * k + 2
    rng = np.random.RandomState(seed)
    # distinct rows per query in no order, as the top-k gives them; row n_truth - 1 stays free for "outside"
    rows = np.argsort(rng.rand(n_queries, n_truth - 1), axis=1)[:, :k].astype(np.int32)
    if ties == "none":
        probabilities = rng.permutation(n_queries * k).reshape(n_queries, k).astype(np.float32) / np.float32(n_queries * k)
    elif ties == "some":
        probabilities = (rng.randint(0, max(2, k // 2), size=(n_queries, k)) / np.float32(max(2, k // 2))).astype(np.float32)
    elif ties == "all":
        probabilities = np.repeat(rng.rand(n_queries).astype(np.float32)[:, None], k, axis=1)
    else:
        probabilities = np.full((n_queries, k), 0.25, dtype=np.float32)
    probabilities = np.ascontiguousarray(probabilities, dtype=np.float32)
    ratios = rng.randint(0, 101, size=(n_queries, k)).astype(np.uint8)
    exact = np.full(n_queries, -1, dtype=np.int32)
    best = np.full(n_queries, -1, dtype=np.int32)
    for q in range(n_queries):
        kind = q % 8
        a, b = rng.randint(0, k), rng.randint(0, k)
        if kind == 1:
            exact[q] = rows[q, a]
        elif kind == 2:
            exact[q] = n_truth - 1
        elif kind == 3:
            exact[q] = rows[q, a]
            best[q] = rows[q, b]
        elif kind == 4:
            best[q] = rows[q, a]
        elif kind == 5:
            rows[q, a] = -1
            rows[q, b] = n_truth + rng.randint(0, 5) if b != a else -1
        elif kind == 6:
            exact[q] = rows[q, a]
            rows[q, b] = rows[q, a]
            rows[q, rng.randint(0, k)] = -7
        elif kind == 7:
            rows[q] = np.where(rng.rand(k) < 0.5, -1, n_truth + 3)
            best[q] = n_truth - 1
        if exact[q] >= 0 and kind != 3:
            best[q] = exact[q]
    return rows, probabilities, ratios, exact, best
