"""The duplicate-groups stage restated in NumPy: the link rule of ds_duplicate_links_device slot by slot, a sequential
union-find for the components, and the link sets the kernel tests share -- the shapes where a concurrent union-find goes
wrong.  A plain module like sweep_cases.py: no fixtures, no GPU.

A call is (q_first, rows int32[Q, k], ratios uint8[Q, k], probabilities float32[Q, k] or None, exact int32[Q] or None):
the arguments of one ds_duplicate_links_device call on query rows [q_first, q_first + Q) of the truth table.
"""
import numpy as np


def links_of(rows, ratios, probabilities, exact, q_first, n_truth, t, u):
    """(edges int64[E, 2], reasons uint8[Q, k], counts int64[3]) of one call at Levenshtein threshold t and probability
    threshold u.  A slot is skipped when its row is negative, >= n_truth or the query's own row; close = ratio > t, model =
    probability > u as float32 (a NaN is not above); reason = close | model << 1.  The edges are (own row, other row): per
    query the exact link first (exact[q] in range and not the own row), then its slots with a non-zero reason in order.
    counts = exact links, close slots, slots with model and not close."""
    rows = np.asarray(rows).astype(np.int64)
    n_queries, k = rows.shape
    own = q_first + np.arange(n_queries, dtype=np.int64)
    valid = (rows >= 0) & (rows < n_truth) & (rows != own[:, None])
    close = valid & (np.asarray(ratios).astype(np.int64) > int(t))
    if probabilities is None:
        model = np.zeros_like(valid)
    else:
        with np.errstate(invalid="ignore"):
            model = valid & (np.asarray(probabilities, dtype=np.float32) > np.float32(u))
    reasons = (close.astype(np.uint8) | (model.astype(np.uint8) << 1)).astype(np.uint8)
    if exact is None:
        linked = np.zeros(0, dtype=np.int64)
        exact = np.zeros(n_queries, dtype=np.int64)
    else:
        exact = np.asarray(exact).astype(np.int64)
        linked = np.nonzero((exact >= 0) & (exact < n_truth) & (exact != own))[0]
    query, slot = np.nonzero(reasons)
    order = np.argsort(np.concatenate((linked * (k + 1), query * (k + 1) + slot + 1)), kind="stable")
    edges = np.stack((np.concatenate((own[linked], own[query])), np.concatenate((exact[linked], rows[query, slot]))),
                     axis=1)[order]
    counts = np.array([linked.shape[0], close.sum(), (model & ~close).sum()], dtype=np.int64)
    return edges.reshape(-1, 2), reasons, counts


def link_columns(rows, ratios, probabilities, exact, q_first, n_truth, t, u, title_ids):
    """The columns of duplicate_groups' `links` for one call, as a dict of arrays in the order and with the dtypes of
    LINK_COLUMNS: per query one wide line [exact link, slot 0, ..., slot k-1], kept where the exact row links or the
    slot's reason is non-zero, read off row by row -- so the lines come by row, the exact link first, then by slot.  An
    exact link has ratio 100, probability NaN and stage 1; a slot its own ratio and probability (NaN without
    probabilities) and stage 2 when close, else 3."""
    rows = np.asarray(rows).astype(np.int64)
    n_queries, k = rows.shape
    ids = np.asarray(title_ids, dtype=np.int64)
    own = q_first + np.arange(n_queries, dtype=np.int64)
    _, reasons, _ = links_of(rows, ratios, probabilities, exact, q_first, n_truth, t, u)
    exact = np.full(n_queries, -1, dtype=np.int64) if exact is None else np.asarray(exact).astype(np.int64)
    if probabilities is None:
        probabilities = np.full(rows.shape, np.nan, dtype=np.float32)
    first = lambda column, value, dtype: np.concatenate(
        (np.full((n_queries, 1), value, dtype=dtype), np.asarray(column, dtype=dtype)), axis=1)
    keep = np.concatenate((((exact >= 0) & (exact < n_truth) & (exact != own))[:, None], reasons != 0), axis=1)
    row = np.broadcast_to(own[:, None], keep.shape)[keep]
    match_row = np.concatenate((exact[:, None], rows), axis=1)[keep]
    return {"row": row, "match_row": match_row, "title_id": ids[row], "match_title_id": ids[match_row],
            "levenshtein_ratio": first(ratios, 100, np.uint8)[keep],
            "probability": first(probabilities, np.nan, np.float32)[keep],
            "stage": first(np.where(reasons & 1, 2, 3), 1, np.int8)[keep]}


def components(n, edges):
    """(labels int32[n], sizes int32[n]): the connected components of n rows under `edges`, by a sequential union-find;
    a row's label is the lowest row of its component, its size the rows of that component."""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in np.asarray(edges, dtype=np.int64).reshape(-1, 2).tolist():
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)
    labels = np.array([find(x) for x in range(n)], dtype=np.int32)
    return labels, np.bincount(labels, minlength=n).astype(np.int32)[labels]


def expected(calls, n_truth, t, u):
    """(labels, sizes, [reasons per call], counts) of `calls` accumulated into one forest."""
    edges, reasons, counts = [np.zeros((0, 2), dtype=np.int64)], [], np.zeros(3, dtype=np.int64)
    for q_first, rows, ratios, probabilities, exact in calls:
        if rows.shape[0] == 0:
            reasons.append(np.zeros(rows.shape, dtype=np.uint8))
            continue
        call_edges, call_reasons, call_counts = links_of(rows, ratios, probabilities, exact, q_first, n_truth, t, u)
        edges.append(call_edges)
        reasons.append(call_reasons)
        counts += call_counts
    labels, sizes = components(n_truth, np.concatenate(edges))
    return labels, sizes, reasons, counts


# ---- link sets ------------------------------------------------------------------------------------------------------

T, U = 94, np.float32(0.9)      # the thresholds the builders are written for
CLOSE, FAR = 100, 0             # a ratio above / not above T


def _call(rows, ratios=CLOSE, q_first=0, probabilities=None, exact=None):
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    if np.isscalar(ratios):
        ratios = np.full(rows.shape, ratios, dtype=np.uint8)
    return (q_first, rows, np.ascontiguousarray(ratios, dtype=np.uint8), probabilities, exact)


def chain(n, order="ascending", seed=1):
    """One call, k = 1, whose links form the path 0 - 1 - ... - n-1 (ascending: row i names i + 1; descending: row i names
    i - 1) or a path through the rows in a shuffled order (row p[i] names p[i + 1]).  One row names nothing (-1)."""
    rows = np.full(n, -1, dtype=np.int64)
    if order == "ascending":
        rows[:-1] = np.arange(1, n)
    elif order == "descending":
        rows[1:] = np.arange(n - 1)
    else:
        path = np.random.RandomState(seed).permutation(n)
        rows[path[:-1]] = path[1:]
    return [_call(rows.reshape(n, 1))]


def star(n, centre):
    """One call, k = 1: every row names `centre` (the centre names itself, which is skipped)."""
    return [_call(np.full((n, 1), centre))]


def two_halves_joined_later(half):
    """Two paths of `half` rows each in the first call; one link between them in a second call of one query."""
    rows = np.arange(1, 2 * half + 1).reshape(-1, 1)
    rows[half - 1] = -1
    rows[2 * half - 1] = -1
    bridge = half // 3
    return [_call(rows), _call([[half + half // 2]], q_first=bridge)]


def random_links(n, k, seed, block=None, share=0.2):
    """One call over all n rows of k slots: candidates drawn inside the row's block of `block` rows (None: anywhere), a
    `share` of the slots close, a share above U (some both), the others neither; a few exact rows."""
    rng = np.random.RandomState(seed)
    if block is None:
        rows = rng.randint(0, n, (n, k))
    else:
        base = (np.arange(n) // block * block)[:, None]
        rows = np.minimum(base + rng.randint(0, block, (n, k)), n - 1)
    ratios = np.where(rng.rand(n, k) < share, CLOSE, rng.choice([0, 50, 93, 94], (n, k)))
    probabilities = np.where(rng.rand(n, k) < share, np.float32(0.95), rng.rand(n, k).astype(np.float32) * U)
    probabilities = np.ascontiguousarray(probabilities, dtype=np.float32)
    exact = np.where(rng.rand(n) < 0.02, rng.randint(0, n, n), -1).astype(np.int32)
    return [_call(rows, ratios, probabilities=probabilities, exact=exact)]


def cut(call, pieces):
    """The queries of one call cut into `pieces` consecutive calls (uneven, none empty), each with its own q_first."""
    q_first, rows, ratios, probabilities, exact = call
    n = rows.shape[0]
    bounds = np.unique(np.concatenate(([0, n], (np.arange(1, pieces) * n) // pieces + np.arange(1, pieces) % 3)))
    return [(q_first + a, rows[a:b], ratios[a:b], None if probabilities is None else probabilities[a:b],
             None if exact is None else exact[a:b]) for a, b in zip(bounds[:-1], bounds[1:])]


def dense(n, k=64, block=500, seed=3):
    """Every slot of every row links (ratio 100) to a row of its block: the components are the blocks, almost every union
    finds its two rows joined already."""
    rng = np.random.RandomState(seed)
    base = (np.arange(n) // block * block)[:, None]
    rows = np.minimum(base + rng.randint(0, block, (n, k)), n - 1)
    rows[:, 0] = np.minimum(np.arange(n) + 1, np.minimum(base[:, 0] + block - 1, n - 1))   # the block is connected
    return [_call(rows)]


def twins(n, k=3):
    """All titles identical, seen through the exact rows alone: every row's exact row is the LAST row, no slot links and
    there are no predictions."""
    rows = np.full((n, k), -1)
    return [_call(rows, FAR, exact=np.full(n, n - 1, dtype=np.int32))]


def nothing(n, k=4, seed=5):
    """Candidates everywhere, none of them close or above U, no exact row."""
    rng = np.random.RandomState(seed)
    rows = rng.randint(0, n, (n, k))
    probabilities = np.ascontiguousarray(rng.rand(n, k).astype(np.float32) * U)
    return [_call(rows, rng.choice([0, 60, 94], (n, k)), probabilities=probabilities, exact=np.full(n, -1, dtype=np.int32))]


def edge_slots(n=300):
    """Rows 0..7 with k = 8 whose slots hold what must be skipped (negative, >= n, the own row) with a ratio of 100 and a
    probability of 1, beside ratios at T and one above it and probabilities at U, one ulp above it, NaN and infinite.  The
    exact rows: out of range on both sides, the own row, and one real link."""
    k = 8
    rows = np.full((8, k), -1, dtype=np.int64)
    ratios = np.full((8, k), CLOSE, dtype=np.uint8)
    probabilities = np.ones((8, k), dtype=np.float32)
    rows[0] = [-1, -2, -(2 ** 31), n, n + 1, 2 ** 31 - 1, 0, -7]               # nothing links
    rows[1] = [1, 1, n, 1, -1, 1, 1, 1]                                         # itself only
    rows[2] = np.arange(10, 18)                                                 # ratios around T, probabilities low
    ratios[2] = [T, T + 1, T - 1, 0, 100, T, 255, T]
    probabilities[2] = 0
    rows[3] = np.arange(20, 28)                                                 # probabilities around U, ratios low
    ratios[3] = 0
    probabilities[3] = [U, np.nextafter(U, np.float32(1)), np.nextafter(U, np.float32(0)), np.nan, np.inf, -np.inf, 0, 1]
    rows[4] = [30, 30, 31, 31, 4, 4, 32, 32]                                    # repeats, both reasons at once
    ratios[4] = [100, 0, 100, 0, 100, 100, 0, 0]
    probabilities[4] = [1, 1, 0, 0, 1, 1, np.nan, 1]
    rows[5:8] = np.arange(40, 64).reshape(3, 8)
    ratios[5:8] = 0
    probabilities[5:8] = np.nan
    exact = np.array([-1, 1, n, -5, 299, 2 ** 31 - 1, 6, 50], dtype=np.int32)
    return [_call(rows, ratios, probabilities=probabilities, exact=exact)]
