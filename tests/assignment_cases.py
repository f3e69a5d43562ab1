"""One-to-one matches ("One-to-one matches"): the rule restated twice, and the cases.

The inputs are the ranked slots of the rank stage, [Q, n]: row int32, probability float32, ratio uint8, stage int8.
`edge_keys` restates which slots are edges and their keys, `deferred_acceptance` the matching as the textbook states it
(one title at a time, a displaced title goes on at once), `greedy` the sorted loop that equals it where every title's edges
descend in score, `is_stable` the definition of the result.  None of them shares code with the kernels.

A case is a function that returns a Case; the empty slot of the rank stage is (row -1, NaN, ratio 0, stage 0)."""
import collections

import numpy as np

Case = collections.namedtuple("Case", ("row", "probability", "ratio", "stage", "n_truth", "threshold"))
Result = collections.namedtuple("Result", ("match_row", "match_slot", "first_row", "counts"))
TITLE_MASK = (1 << 31) - 1
THRESHOLD = np.float32(0.9)


def edge_keys(row, probability, ratio, stage, q_first, n_truth, threshold):
    """uint64[Q, n]: class << 62 | payload << 31 | (2^31 - 1 - q), 0 for a slot that is no edge."""
    row, stage = np.asarray(row, dtype=np.int64), np.asarray(stage, dtype=np.int64)
    probability = np.asarray(probability, dtype=np.float32)
    bits = probability.view(np.uint32).astype(np.uint64)
    with np.errstate(invalid="ignore"):
        above = probability > np.float32(threshold)                      # a NaN is not above
    model = (stage == 3) & above & (bits >> np.uint64(31) == 0)
    eligible = (row >= 0) & (row < n_truth) & ((stage == 1) | (stage == 2) | model)
    edge = eligible.copy()
    for s in range(1, row.shape[1]):                                    # no earlier slot of the title is an edge to the row
        edge[:, s] &= ~((row[:, :s] == row[:, s:s + 1]) & eligible[:, :s]).any(axis=1)
    klass = np.select([stage == 1, stage == 2], [3, 2], 1).astype(np.uint64)
    payload = np.select([stage == 1, stage == 2], [np.zeros_like(bits), np.asarray(ratio).astype(np.uint64)], bits)
    title = (TITLE_MASK - (q_first + np.arange(row.shape[0], dtype=np.int64))).astype(np.uint64)
    keys = (klass << np.uint64(62)) | (payload << np.uint64(31)) | title[:, None]
    return np.where(edge, keys, np.uint64(0))


def keys_of(case, q_first=0):
    return edge_keys(case.row, case.probability, case.ratio, case.stage, q_first, case.n_truth, case.threshold)


def _edges(rows, keys, n_truth):
    rows, keys = np.asarray(rows), np.asarray(keys)
    return (keys != 0) & (rows >= 0) & (rows < n_truth)


def _result(rows, edge, match_slot):
    count, n = rows.shape
    match_slot = np.asarray(match_slot, dtype=np.int32)
    matched = match_slot >= 0
    match_row = np.where(matched, rows[np.arange(count), np.maximum(match_slot, 0)], -1).astype(np.int32)
    first_row = np.where(edge.any(axis=1), rows[np.arange(count), edge.argmax(axis=1)], -1).astype(np.int32) if n else \
        np.full(count, -1, np.int32)
    displaced = (first_row >= 0) & (match_row != first_row)
    counts = np.array([edge.sum(), matched.sum(), displaced.sum(), (displaced & ~matched).sum()], dtype=np.int64)
    return Result(match_row, match_slot, first_row, counts)


def deferred_acceptance(rows, keys, n_truth, order=None):
    """The titles propose one at a time, in `order` (default: as numbered); a truth row keeps the larger key, and the title
    it lets go proposes on at once, from the slot after the one it lost."""
    rows, keys = np.asarray(rows), np.asarray(keys)
    count, n = rows.shape
    edge = _edges(rows, keys, n_truth).tolist()
    row_list, key_list = rows.tolist(), keys.tolist()
    held, holder = [0] * n_truth, [-1] * n_truth
    standing = [0] * count
    for start in (range(count) if order is None else order):
        q = int(start)
        while q >= 0:
            s = standing[q]
            while s < n and not (edge[q][s] and key_list[q][s] > held[row_list[q][s]]):
                s += 1
            standing[q] = s
            if s == n:
                break
            t = row_list[q][s]
            q, held[t], holder[t] = holder[t], key_list[q][s], q
    return _result(rows, np.asarray(edge, dtype=bool).reshape(count, n), [s if s < n else -1 for s in standing])


def greedy(rows, keys, n_truth):
    """All edges by (class, payload) descending, then title ascending, then slot ascending; an edge is taken when its title
    and its row are both still free."""
    rows, keys = np.asarray(rows), np.asarray(keys)
    count, n = rows.shape
    edge = _edges(rows, keys, n_truth)
    query, slot = np.nonzero(edge)
    score = (keys[query, slot] >> np.uint64(31)).astype(np.int64)
    order = np.lexsort((slot, query, -score))
    match_slot = np.full(count, -1, dtype=np.int32)
    taken = np.zeros(max(n_truth, 1), dtype=bool)
    for q, s in zip(query[order].tolist(), slot[order].tolist()):
        t = rows[q, s]
        if match_slot[q] < 0 and not taken[t]:
            match_slot[q], taken[t] = s, True
    return _result(rows, edge, match_slot)


def is_descending(rows, keys, n_truth):
    """Do every title's edges come in descending (class, payload) order -- what the rank stage guarantees?"""
    edge = _edges(rows, keys, n_truth)
    score = np.where(edge, np.asarray(keys) >> np.uint64(31), np.uint64(0)).astype(np.int64)
    for q in range(score.shape[0]):
        mine = score[q][edge[q]]
        if (np.diff(mine) > 0).any():
            return False
    return True


def is_stable(rows, keys, n_truth, match_row, match_slot):
    """The definition: a matching over edges, one title per row at most, and no edge (q, t) outside it such that q prefers t
    to what it got (an earlier slot, or q unmatched) while t's key for q is above the key t holds (or t is free)."""
    rows, keys = np.asarray(rows), np.asarray(keys)
    edge = _edges(rows, keys, n_truth)
    count, n = rows.shape
    held = np.zeros(max(n_truth, 1), dtype=np.uint64)
    for q in range(count):
        s = int(match_slot[q])
        if s < 0:
            if match_row[q] != -1:
                return False
            continue
        if not (s < n and edge[q, s] and rows[q, s] == match_row[q]) or held[match_row[q]] != 0:
            return False
        held[match_row[q]] = keys[q, s]
    for q, s in zip(*np.nonzero(edge)):
        prefers = match_slot[q] < 0 or s < match_slot[q]
        if prefers and keys[q, s] > held[rows[q, s]]:
            return False
    return True


def expected(case, q_first=0):
    return deferred_acceptance(case.row, keys_of(case, q_first), case.n_truth)


# ---- the cases -----------------------------------------------------------------------------------------------------------

def _empty(count, n):
    return (np.full((count, n), -1, np.int32), np.full((count, n), np.nan, np.float32), np.zeros((count, n), np.uint8),
            np.zeros((count, n), np.int8))


def _model(slots, q, s, row, probability, ratio=50):
    slots[0][q, s], slots[1][q, s], slots[2][q, s], slots[3][q, s] = row, probability, ratio, 3


def _head(slots, q, row, stage, ratio):
    slots[0][q, 0], slots[1][q, 0], slots[2][q, 0], slots[3][q, 0] = row, 1.0, ratio, stage


def no_contention(count=1000, n=3):
    """Every title has n rows of its own: everybody gets slot 0."""
    slots = _empty(count, n)
    for s, p in enumerate((0.99, 0.95, 0.92)[:n]):
        slots[0][:, s] = np.arange(count) * n + s
        slots[1][:, s], slots[2][:, s], slots[3][:, s] = p, 60 - s, 3
    return Case(*slots, count * n, THRESHOLD)


def best_claimant():
    """What one round of "every row keeps its best claimant" gets wrong: q0 -> t1 (0.99), t0 (0.95); q1 -> t0 (0.90);
    q2 -> t1 (0.995).  q2 takes t1 from q0, whose second choice then takes t0 from q1."""
    slots = _empty(3, 2)
    _model(slots, 0, 0, 1, 0.99)
    _model(slots, 0, 1, 0, 0.95)
    _model(slots, 1, 0, 0, 0.90)
    _model(slots, 2, 0, 1, 0.995)
    return Case(*slots, 2, np.float32(0.5))


def chain(length=300):
    """Title 0 holds row 0 by an exact match.  Title i = 1..L has (row i - 1, w_i), (row i, v_i) with
    w_1 > v_1 > w_2 > v_2 > ...: title 1 loses row 0, its second slot takes row 1 from title 2, and so on down the chain.
    Every title ends on its second slot, the last one on a row nobody else wants."""
    slots = _empty(length + 1, 2)
    _head(slots, 0, 0, 1, 100)
    score = (np.float32(0.99) - np.arange(2 * length, dtype=np.float32) * np.float32(1e-4)).astype(np.float32)
    for i in range(1, length + 1):
        _model(slots, i, 0, i - 1, score[2 * (i - 1)])
        _model(slots, i, 1, i, score[2 * (i - 1) + 1])
    return Case(*slots, length + 1, THRESHOLD)


def classes():
    """One slot per title, several titles per row.  row 0: exact, close at 100, model at 1.0; row 1: close 97, close 95;
    row 2: a probability and the next float32 above it; row 3: the same probability twice; row 4: the same ratio twice;
    row 5: exact twice.  The winners are titles 0, 3, 6, 7, 9, 11."""
    p = np.float32(0.95)
    slots = _empty(13, 1)
    _model(slots, 2, 0, 0, 1.0, 100)
    _head(slots, 1, 0, 2, 100)
    _head(slots, 0, 0, 1, 100)
    _head(slots, 4, 1, 2, 95)
    _head(slots, 3, 1, 2, 97)
    _model(slots, 5, 0, 2, p)
    _model(slots, 6, 0, 2, np.nextafter(p, np.float32(1)))
    _model(slots, 7, 0, 3, p)
    _model(slots, 8, 0, 3, p)
    _head(slots, 9, 4, 2, 96)
    _head(slots, 10, 4, 2, 96)
    _head(slots, 11, 5, 1, 100)
    _head(slots, 12, 5, 1, 100)
    return Case(*slots, 6, THRESHOLD)


CLASS_WINNERS = (0, 3, 6, 7, 9, 11)


def eligibility(threshold=THRESHOLD):
    """Four slots per title, every title on rows of its own (4 q .. 4 q + 3), so that a title's answer shows which of its
    slots are edges.  Per title: (slots, the slot it must end on or -1)."""
    up, down = np.nextafter(threshold, np.float32(2)), np.nextafter(threshold, np.float32(-2))
    nan = np.float32(np.nan)
    n_titles = 12
    n_truth = 4 * n_titles
    # (row offset or absolute marker, probability, stage) per slot; row None: -1, "end": n_truth, int: 4 q + that
    plans = [
        ([(0, threshold, 3), (1, up, 3)], 1),                              # at the threshold: out; one ulp above: in
        ([(0, down, 3), (1, up, 3)], 1),                                   # one ulp below: out
        ([(0, nan, 3), (1, np.float32(-0.0), 3), (2, np.float32(0.95), 3)], 2),     # NaN, -0.0: out
        ([(0, np.float32(0.99), 0), (1, np.float32(0.99), 3)], 1),          # stage 0: out, whatever it holds
        ([(None, np.float32(0.99), 3), ("end", np.float32(0.99), 3), (2, np.float32(0.95), 3)], 2),    # rows -1, n_truth
        ([(None, np.float32(1.0), 1), ("end", np.float32(1.0), 2), (3, np.float32(0.91), 3)], 2),      # also as heads
        ([(0, np.float32(0.5), 3), (0, np.float32(0.99), 3)], 1),           # the first was no edge: the repeat is one
        ([(0, threshold, 3), (1, threshold, 3), (2, down, 3), (3, nan, 3)], -1),   # no edge at all
        ([(0, np.float32(0.99), 4), (1, np.float32(0.99), -1), (2, np.float32(0.99), 3)], 2),          # unknown stages
        ([(0, np.float32(np.inf), 3)], 0),                                 # +inf is above and its sign is clear
        ([(0, np.float32(-np.inf), 3), (1, np.float32(-1.0), 3)], -1),
        ([(0, np.float32(0.5), 2)], 0),                                    # a close head needs no probability
    ]
    assert len(plans) == n_titles
    slots = _empty(n_titles, 4)
    for q, (plan, _) in enumerate(plans):
        for s, (row, probability, stage) in enumerate(plan):
            slots[0][q, s] = -1 if row is None else n_truth if row == "end" else 4 * q + row
            slots[1][q, s], slots[2][q, s], slots[3][q, s] = probability, 90, stage
    return Case(*slots, n_truth, np.float32(threshold)), np.array([slot for _, slot in plans], dtype=np.int32)


def negative_threshold():
    """Below zero the sign test decides: -0.0 and -0.25 are above -0.5 and still no edges; +0.0 is one."""
    slots = _empty(3, 2)
    _model(slots, 0, 0, 0, np.float32(-0.0))
    _model(slots, 0, 1, 1, np.float32(0.0))
    _model(slots, 1, 0, 2, np.float32(-0.25))
    _model(slots, 1, 1, 3, np.float32(0.25))
    _model(slots, 2, 0, 4, np.float32(-0.75))
    return Case(*slots, 5, np.float32(-0.5)), np.array([1, 1, -1], dtype=np.int32)


def repeated_rows():
    """A row repeated inside a title is an edge once.  Title 0: row 0 three times (0.99, 0.97, 0.95) then row 1; title 1
    takes row 0 with an exact match: title 0 must go on to row 1, not stand on row 0 again."""
    slots = _empty(2, 4)
    for s, p in enumerate((0.99, 0.97, 0.95)):
        _model(slots, 0, s, 0, p)
    _model(slots, 0, 3, 1, 0.93)
    _head(slots, 1, 0, 1, 100)
    return Case(*slots, 2, THRESHOLD)


def unordered(count=2000, seed=5):
    """Ascending probabilities: slot order is the title's preference all the same.  The first two titles are an instance
    where the sorted loop differs: q0 -> t0 (0.91), t1 (0.99); q1 -> t1 (0.95).  q0 keeps t0 and q1 gets t1; the sorted
    loop gives t1 to q0 and leaves q1 with nothing."""
    rng = np.random.RandomState(seed)
    n, n_truth = 3, count // 2
    slots = _empty(count, n)
    values = np.sort(rng.choice(np.linspace(0.905, 0.995, 40).astype(np.float32), size=(count, n)), axis=1)
    slots[0][:], slots[1][:], slots[2][:], slots[3][:] = rng.randint(2, n_truth, (count, n)), values, 70, 3
    for q in (0, 1):
        slots[0][q], slots[1][q], slots[2][q], slots[3][q] = -1, np.nan, 0, 0
    _model(slots, 0, 0, 0, 0.91)
    _model(slots, 0, 1, 1, 0.99)
    _model(slots, 1, 0, 1, 0.95)
    return Case(*slots, n_truth, THRESHOLD)


def hot_row(count=5000, seed=9):
    """Every title wants row 0 first; the second and third slots are drawn from 64 rows."""
    rng = np.random.RandomState(seed)
    slots = _empty(count, 3)
    values = -np.sort(-rng.choice(np.linspace(0.91, 0.99, 9).astype(np.float32), size=(count, 3)), axis=1)
    slots[0][:, 0] = 0
    slots[0][:, 1:] = rng.randint(1, 65, (count, 2))
    slots[1][:], slots[2][:], slots[3][:] = values, 80, 3
    return Case(*slots, 65, THRESHOLD)


def random_ties(count=20000, n=5, n_truth=5000, seed=17):
    """What the rank stage leaves: an exact or a close head on some titles, then model slots by probability descending, from
    16 distinct values of which some lie at or below the threshold; a few rows repeat inside a title, some titles are short."""
    rng = np.random.RandomState(seed)
    slots = _empty(count, n)
    values = np.linspace(0.87, 0.99, 16).astype(np.float32)
    values[4] = THRESHOLD                                               # a value exactly at the threshold
    slots[0][:] = rng.randint(0, n_truth, (count, n))
    slots[1][:] = -np.sort(-rng.choice(values, size=(count, n)), axis=1)
    slots[2][:] = rng.randint(30, 95, (count, n))
    slots[3][:] = 3
    kind = rng.randint(0, 10, count)
    exact, close = kind == 0, kind == 1
    slots[1][exact | close, 0] = 1.0
    slots[2][exact, 0], slots[3][exact, 0] = 100, 1
    slots[2][close, 0], slots[3][close, 0] = rng.randint(95, 101, int(close.sum())), 2
    filled = rng.randint(0, n + 1, count)
    filled[rng.rand(count) < 0.7] = n
    cut = np.arange(n)[None, :] >= filled[:, None]
    slots[0][cut], slots[1][cut], slots[2][cut], slots[3][cut] = -1, np.nan, 0, 0
    return Case(*slots, n_truth, THRESHOLD)


def small(count, n, n_truth, seed=3):
    """Random model slots for the sizes at the edges: one truth row, one slot, no title, one title."""
    rng = np.random.RandomState(seed)
    slots = _empty(count, n)
    if count:
        slots[0][:] = rng.randint(0, n_truth, (count, n))
        slots[1][:] = -np.sort(-rng.choice(np.linspace(0.88, 0.99, 12).astype(np.float32), size=(count, n)), axis=1)
        slots[2][:], slots[3][:] = 50, 3
    return Case(*slots, n_truth, THRESHOLD)


def cut(case, at):
    """The case's slots as chunks cut at the given titles: [(q_first, row, probability, ratio, stage), ...]."""
    bounds = [0] + [a for a in at if 0 < a < case.row.shape[0]] + [case.row.shape[0]]
    return [(first, *(a[first:last] for a in case[:4])) for first, last in zip(bounds[:-1], bounds[1:])]


ALL = {"no_contention": no_contention, "best_claimant": best_claimant, "chain": chain, "classes": classes,
       "eligibility": lambda: eligibility()[0], "negative_threshold": lambda: negative_threshold()[0],
       "repeated_rows": repeated_rows, "unordered": unordered, "hot_row": hot_row, "random_ties": random_ties,
       "n_truth_1": lambda: small(200, 3, 1), "n_1": lambda: small(300, 1, 40), "no_title": lambda: small(0, 3, 10),
       "one_title": lambda: small(1, 4, 10), "odd_count": lambda: small(1000 + 37, 2, 300)}
