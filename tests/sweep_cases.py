"""The threshold sweep restated in NumPy from what the oracle already has, cell by cell: the close ratio read at a
threshold from its three parts, `title_cases.best_from_ratios`, `oracle.select_matches`, an exact look-up and the four
counters of cli.py:107-120.  Plus the synthetic queries the kernel tests share.  A plain module like ranked_cases.py: no
fixtures, no GPU; the functions that need the oracle take it as an argument.
"""
import numpy as np

import title_cases as tc

COUNTERS = ("correctly_matched", "incorrectly_matched", "correctly_not_found", "incorrectly_not_found")
MAX_T, MAX_U = 101, 256


# ---- the close ratio taken apart ------------------------------------------------------------------------------------

def prefilter_floor(x_len, y_len):
    """d: the floor of predict.py:141-151's value, ((lx + ly - |lx - ly|) / (lx + ly)) * 100 in float64 in that order;
    100 for two empty titles (0 / 0 is NaN, which is below no threshold)."""
    lx, ly = np.asarray(x_len).astype(np.int64), np.asarray(y_len).astype(np.int64)
    total, delta = lx + ly, np.abs(lx - ly)
    value = ((total - delta).astype(np.float64) / np.maximum(total, 1).astype(np.float64)) * 100
    return np.where(total == 0, 100, np.floor(value)).astype(np.uint8)


def token_sort(codes, space, sort_key):
    """' '.join(sorted(text.split())) of common.py:166 on a code array; sort_key[code] is the character's order."""
    words, word = [], []
    for code in list(codes) + [space]:
        if code == space:
            if word:
                words.append(word)
            word = []
        else:
            word.append(int(code))
    words.sort(key=lambda w: [int(sort_key[c]) for c in w])
    out = []
    for i, w in enumerate(words):
        out += ([space] if i else []) + w
    return np.array(out, dtype=np.uint8)


def close_parts(oracle, x_len, y_len, x_enc, y_enc, space, sort_key):
    """(d, r, s) uint8[n] of n padded pairs, nothing skipped: r = common.levenshtein_ratio, s =
    common.levenshtein_token_sort_ratio (the oracle's rounded ratio on the titles and on their token-sorted forms)."""
    d = prefilter_floor(x_len, y_len)
    # at threshold -1 the pre-filter passes everything and every ratio is above it: close_ratios returns r
    r = oracle.close_ratios(x_len, y_len, x_enc, y_enc, space, sort_key, threshold=-1)
    s = np.empty_like(r)
    for i in range(r.shape[0]):
        s[i] = oracle.levenshtein_ratio_rounded(token_sort(x_enc[i, :x_len[i]], space, sort_key),
                                                token_sort(y_enc[i, :y_len[i]], space, sort_key))
    return d, r, s


def skipped_parts(d, r, s, t_min, t_max):
    """What ds_close_parts_device leaves of (d, r, s) for thresholds [t_min, t_max]: r and s are 0 where d < t_min, s is 0
    where r > t_max."""
    dead = d < t_min
    r = np.where(dead, 0, r).astype(np.uint8)
    return d, r, np.where(dead | (r > t_max), 0, s).astype(np.uint8)


def value_at(d, r, s, t):
    """Prediction._get_levenshtein_ratio (predict.py:147-156) at the integer threshold t from the three parts."""
    d, r, s = (np.asarray(a).astype(np.int64) for a in (d, r, s))
    return np.where(t > d, 0, np.where(r > t, r, s)).astype(np.uint8)


def case_parts(oracle, case, pair_q, pair_t, sort_key, space=tc.SPACE):
    """(d, r, s) of the pairs of a title_cases.Case, 0 for a pair outside the tables (as tc.expected_ratios)."""
    valid = tc.valid_pairs(case, pair_q, pair_t)
    q = np.where(valid, pair_q, 0).astype(np.int64)
    t = np.where(valid, pair_t, 0).astype(np.int64)
    parts = close_parts(oracle, case.q_len[q], case.t_len[t], tc.rows255(case.q_enc)[q], tc.rows255(case.t_enc)[t], space,
                        sort_key)
    return tuple(np.where(valid, part, 0).astype(np.uint8) for part in parts)


def close_pairs(case):
    """The pairs the CPU and the GPU test of the parts share: 300 queries x 10 hostile candidate rows, and every special
    title against every special title (empty, spaces only, 128 words, codes >= 64)."""
    rows = tc.make_rows(case, 0, 300, 10, seed=2010)
    pair_q, pair_t = tc.pairs_of_rows(rows, 0)
    q_special = tc.special_rows(case.q_enc, case.q_len, case.q_large)
    t_special = tc.special_rows(case.t_enc, case.t_len, case.t_large)
    return (np.concatenate((pair_q, np.repeat(q_special, t_special.shape[0]))).astype(np.int64),
            np.concatenate((pair_t, np.tile(t_special, q_special.shape[0]))).astype(np.int64))


# ---- the rule, cell by cell -----------------------------------------------------------------------------------------

def predictions_of(oracle, rows, d, r, s, probabilities, exact, lev, prob):
    """int64[T, U, Q]: the truth row every query gets at every cell, -1 for none: the exact row, else the close row of
    best_from_ratios on the ratios at t, else the row of select_matches at u."""
    rows = np.asarray(rows)
    n_queries, k = rows.shape
    pair_q = np.repeat(np.arange(n_queries), k)
    close = np.stack([tc.best_from_ratios(value_at(d, r, s, int(t)), rows, int(t)) for t in lev]).astype(np.int64)
    model = np.stack([oracle.select_matches(pair_q, rows.reshape(-1), probabilities, k, threshold=u)[1]
                      for u in prob]).astype(np.int64)
    exact = np.asarray(exact).astype(np.int64)
    later = np.where(close[:, None, :] >= 0, close[:, None, :], model[None, :, :])
    return np.where(exact[None, None, :] >= 0, exact[None, None, :], np.where(later >= 0, later, -1))


def count_outcomes(predictions, actual):
    """int64[..., 4] from predictions int64[..., Q]: the loop of cli.py:107-120, one counter per outcome."""
    actual = np.asarray(actual).astype(np.int64)
    found, same = predictions != -1, predictions == actual
    return np.stack([(found & same).sum(-1), (found & ~same).sum(-1), (~found & same).sum(-1),
                     (~found & ~same).sum(-1)], axis=-1).astype(np.int64)


def sweep_counts(oracle, queries, lev, prob):
    """int64[T, U, 4]: what ds_threshold_sweep_device adds for `queries` (a tuple as make_queries returns)."""
    rows, d, r, s, probabilities, exact, actual = queries
    if rows.shape[0] == 0:
        return np.zeros((len(lev), len(prob), 4), dtype=np.int64)
    return count_outcomes(predictions_of(oracle, rows, d, r, s, probabilities, exact, lev, prob), actual)


# ---- synthetic queries ----------------------------------------------------------------------------------------------

LEVELS = np.array([0.0, 0.1, 0.25, 0.3, 0.5, 0.6, 0.75, 0.9, 0.95, 0.99, 1.0], dtype=np.float32)
GRID_3X7 = (np.array([50, 90, 94], dtype=np.int32), np.array([0.1, 0.25, 0.5, 0.75, 0.9, 0.95, 0.99], dtype=np.float32))
CRAFTED = 7                    # queries of crafted_queries
CRAFTED_ROWS = 100             # their rows are below this


def crafted_queries(k):
    """Seven queries of k >= 5 candidates (the ones behind the fifth never count: all parts 0, probability 0, rows of
    their own), written for GRID_3X7.  tests/test_sweep_cpu.py holds what each of them must get."""
    assert k >= 5
    rows = np.arange(CRAFTED * k, dtype=np.int32).reshape(CRAFTED, k) % 50 + 50
    rows[:, :5] = np.arange(CRAFTED * 5, dtype=np.int32).reshape(CRAFTED, 5)          # rows 0..34, all different
    d = np.zeros((CRAFTED, k), dtype=np.uint8)
    r, s = d.copy(), d.copy()
    p = np.zeros((CRAFTED, k), dtype=np.float32)
    exact = np.full(CRAFTED, -1, dtype=np.int32)
    actual = np.full(CRAFTED, -1, dtype=np.int32)
    # 0: an exact row, which is the actual one: right in every cell whatever the candidates say
    exact[0], actual[0] = 77, 77
    d[0, 0], r[0, 0], p[0, 1] = 100, 99, 0.99
    # 1: two candidates tied at the close maximum: no close match; the model's row 7 at 0.8 is right where u < 0.8
    d[1, :2], r[1, :2] = 100, 97
    p[1, :3] = 0.3, 0.3, 0.8
    actual[1] = rows[1, 2]
    # 2: candidate 0 counts through r (60) at t = 50 and through s (96) at 90 and 94; candidate 1 (r = 70) beats it at 50
    # only.  The actual row is candidate 0's: wrong at t = 50, right at 90 and 94
    d[2, :2] = 100
    r[2, :2], s[2, :2] = (60, 70), (96, 0)
    actual[2] = rows[2, 0]
    # 3: two candidates tied at the maximum probability: no match anywhere, and there is none to find
    p[3, :3] = 0.95, 0.5, 0.95
    # 4: a single maximum equal to a threshold (0.5): above 0.1 and 0.25 only; the actual row is another one
    p[4, :2] = 0.5, 0.25
    actual[4] = rows[4, 1]
    # 5: a close match (99 at every t of the grid) for a title that has no match
    d[5, 3], r[5, 3] = 100, 99
    # 6: the pre-filter's value is 80: r = 99 counts at t = 50, nothing at 90 and 94, where the model decides (row of
    # candidate 1 at 0.9: above 0.1 .. 0.75); the actual row is the close one
    d[6, 0], r[6, 0], s[6, 0] = 80, 99, 99
    p[6, 1] = 0.9
    actual[6] = rows[6, 0]
    return rows, d, r, s, p, exact, actual


def make_queries(n_queries, k, n_truth, seed, crafted=True):
    """(rows int32[Q, k], d, r, s uint8[Q, k], probabilities float32[Q, k], exact int32[Q], actual int32[Q]): seeded
    queries whose parts sit around the high thresholds and whose probabilities come from a few levels (ties, values equal
    to a threshold), one in eight with an exact row, one in three with no actual row; the others' actual row is the
    exact one, a candidate's or any row.  With `crafted` and k >= 5 the first queries are crafted_queries(k)."""
    rng = np.random.RandomState(seed)
    rows = rng.randint(0, n_truth, (n_queries, k)).astype(np.int32)
    d = rng.choice(np.array([100, 100, 97, 95, 90, 60], dtype=np.uint8), (n_queries, k))
    r = rng.choice(np.array([0, 40, 80, 91, 95, 96, 100], dtype=np.uint8), (n_queries, k))
    s = rng.choice(np.array([0, 50, 85, 93, 95, 97, 100], dtype=np.uint8), (n_queries, k))
    quiet = rng.rand(n_queries) < 0.6                                   # most queries have no close candidate at all
    r[quiet], s[quiet] = r[quiet] // 3, s[quiet] // 3
    p = LEVELS[rng.randint(0, LEVELS.shape[0], (n_queries, k))]
    fine = rng.rand(n_queries) < 0.5                                    # half of the queries: probabilities of their own
    p[fine] = rng.rand(int(fine.sum()), k).astype(np.float32)
    exact = np.where(rng.rand(n_queries) < 0.125, rng.randint(0, n_truth, n_queries), -1).astype(np.int32)
    kind = rng.randint(0, 6, n_queries)
    candidate = rows[np.arange(n_queries), rng.randint(0, k, n_queries)]
    best = rows[np.arange(n_queries), p.argmax(axis=1)]
    actual = np.select([kind < 2, kind == 2, kind == 3, kind == 4], [-1, candidate, best, np.where(exact >= 0, exact, best)],
                       rng.randint(0, n_truth, n_queries)).astype(np.int32)
    out = [rows, d, r, s, p, exact, actual]
    if crafted and k >= 5:
        for whole, front in zip(out, crafted_queries(k)):
            whole[:CRAFTED] = front[:n_queries]
    return tuple(np.ascontiguousarray(a) for a in out)


def grid(T, U):
    """T Levenshtein thresholds ending at 100 (all of 0..100 for T = 101) and U probability thresholds over [0, 1]."""
    lev = np.arange(MAX_T, dtype=np.int32)[MAX_T - T:] if T > 3 else np.array([50, 90, 94], dtype=np.int32)[3 - T:]
    prob = np.linspace(0, 1, U).astype(np.float32) if U > 1 else np.array([0.9], dtype=np.float32)
    return lev, prob
