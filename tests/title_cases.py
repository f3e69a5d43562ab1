"""Hostile title tables and candidate rows for the launch-form tests of the features and close-match kernels
(tests/test_gpu_features_forms.py, tests/test_gpu_close_matches_forms.py), plus what those tests need to know about a
case FROM ITS INPUTS ALONE: which path of `ds_construct_features_kernel` a pair takes, how the kernel cuts a launch into
units, which pairs lie outside the tables.  tests/test_title_cases_cpu.py asserts on the CPU that the committed seeds
reach every path a GPU test is named for.  A plain module like forest_train_oracle.py: no fixtures, no GPU.

Character codes are those of doppel_speller_amd.feature_engineering: 0 = fill, 1 = space, 2.. = letters and digits
(< 64); a code >= 64 never comes out of encode_title, but the kernels take any uint8 and such a title leaves the
bit-parallel path (its match masks have 64 entries).
"""
import numpy as np

SPACE = 1
WORDS = 15
FEATURES = 66
NAN_BITS = 0x7fc00000
INT32_MAX = 2 ** 31 - 1
N_TRUTH = 1000                      # the number_of_truth_titles the word counts are laid around
EDGE_LENGTHS = (0, 1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 253, 254, 255)
# the order of the edge block: an empty title next to a 255-character one, then inwards
_EDGE_ORDER = (0, 255, 1, 254, 2, 253, 3, 129, 31, 128, 32, 127, 33, 65, 63, 64)
STYLES = ("solid", "words", "ragged", "letters", "spaces")
FEATURE_KS = (1, 2, 3, 7, 15, 16, 17, 23, 24, 32, 100, 127)
CLOSE_KS = (1, 3, 10, 17, 100)
CLOSE_THRESHOLDS = (0, 50, 94, 99, 100)


def best_from_ratios(ratios, rows, threshold):
    """predict.py:172-176 restated: per query the single candidate holding the highest ratio above the threshold, -1
    when none is above it or several hold it."""
    best = np.full(ratios.shape[0], -1, dtype=np.int32)
    for q in range(ratios.shape[0]):
        above = ratios[q] > threshold
        if not above.any():
            continue
        top = ratios[q][above].max()
        hits = np.nonzero(ratios[q] == top)[0]
        if hits.shape[0] == 1:
            best[q] = rows[q, hits[0]]
    return best


def pairs_per_unit(k):
    """ds_features.hip `pairs_per_unit`, restated: consecutive pairs one wave works through -- the k candidates of a
    query (k <= 16), a divisor of k between 8 and 16, or 10; 8 for an explicit pair list (k <= 0)."""
    if k <= 0:
        return 8
    if k <= 16:
        return k
    for d in range(16, 7, -1):
        if k % d == 0:
            return d
    return 10


def units_of(n_pairs, k):
    """(units, pairs per unit) of one launch of n_pairs pairs."""
    per_unit = pairs_per_unit(k)
    return -(-n_pairs // per_unit), per_unit


def straddling_units(pair_q, k):
    """How many units of a launch hold pairs of two different query rows (pair_q: the query row of every pair)."""
    pair_q = np.asarray(pair_q)
    units, per_unit = units_of(pair_q.shape[0], k)
    first = np.arange(units) * per_unit
    last = np.minimum(first + per_unit, pair_q.shape[0]) - 1
    return int((pair_q[first] != pair_q[last]).sum())


# ---- titles ---------------------------------------------------------------------------------------------------------

def _letters(rng, n, pool):
    return rng.randint(2, 2 + pool, n).astype(np.uint8)


def make_title(rng, length, style, large, pool=6):
    """One title of exactly `length` codes.  solid: no space; words: a space now and then; ragged: spaces in front, at
    the end and doubled inside; letters: one-letter words; spaces: nothing but spaces.  large: about one code in eight
    (one at least) is >= 64."""
    if style == "spaces":
        return np.full(length, SPACE, dtype=np.uint8)
    title = _letters(rng, length, pool)
    if style == "words" and length > 2:
        title[1:-1][rng.rand(length - 2) < 0.17] = SPACE
    elif style == "ragged" and length > 0:
        lead, tail = rng.randint(1, 4), rng.randint(1, 4)
        title[:lead] = SPACE
        title[length - min(tail, length):] = SPACE
        for at in np.nonzero(rng.rand(length) < 0.12)[0]:
            title[at:at + 2] = SPACE
    elif style == "letters":
        title[1::2] = SPACE
    if large:
        chars = np.nonzero(title != SPACE)[0]
        if chars.shape[0]:
            picked = chars[rng.rand(chars.shape[0]) < 0.125]
            if picked.shape[0] == 0:
                picked = chars[rng.randint(chars.shape[0])][None]
            title[picked] = rng.randint(64, 256, picked.shape[0]).astype(np.uint8)
    return title


def _random_length(rng, max_len):
    band = rng.rand()
    if band < 0.6:
        high = 40
    elif band < 0.85:
        high = 100
    elif band < 0.95:
        high = 200
    else:
        high = 255
    return int(rng.randint(0, min(high, max_len) + 1))


def _edge_block(rng, max_len):
    titles = []
    lengths = [length for length in _EDGE_ORDER if length <= max_len]
    if max_len not in lengths:
        lengths += [max_len, max_len - 1]
    for style in STYLES:
        for large in (False, True):
            if style == "spaces" and large:
                continue
            titles += [make_title(rng, length, style, large) for length in lengths]
    return titles


def _truth_specials(rng, max_len):
    """Word-count and word-length edges of the truth side: 1 / 15 / 16 / 40 / 128 one-letter words, words of 64, 65, 70,
    100 and 200 characters (a word above 64 takes the literal window search even with a small alphabet)."""
    titles = []
    for words in (1, 15, 16, 40, 128):
        length = 2 * words - 1
        if length <= max_len:
            titles.append(make_title(rng, length, "letters", False))
            titles.append(make_title(rng, min(length + 1, max_len), "letters", False))   # a trailing space
            titles.append(make_title(rng, length, "letters", True))
    for word in (64, 65, 70, 100, 200):
        if word + 12 <= max_len:
            head, tail = _letters(rng, 5, 6), _letters(rng, 5, 6)
            titles.append(np.concatenate((head, [SPACE], _letters(rng, word, 6), [SPACE], tail)).astype(np.uint8))
            titles.append(np.concatenate((_letters(rng, word, 6), [SPACE], tail, [SPACE], head)).astype(np.uint8))
    return titles


def _mutate(rng, title, max_len):
    """A truth title close to a query title: a copy, one or two edits, or its words in another order."""
    kind = rng.randint(4)
    out = title.copy()
    if kind == 1 or kind == 2:
        for _ in range(kind):
            if out.shape[0] == 0:
                break
            at = rng.randint(out.shape[0])
            how = rng.randint(3)
            if how == 0 and out.shape[0] > 1:
                out = np.delete(out, at)
            elif how == 1 and out.shape[0] < max_len:
                out = np.insert(out, at, rng.randint(2, 8)).astype(np.uint8)
            else:
                out[at] = rng.randint(2, 8)
    elif kind == 3:
        cuts = np.nonzero(out == SPACE)[0]
        if cuts.shape[0]:
            parts = np.split(out, cuts)                      # every part but the first starts with its space
            words = [parts[0]] + [part[1:] for part in parts[1:]]
            order = rng.permutation(len(words))
            joined = []
            for i, w in enumerate(order):
                if i:
                    joined.append(np.array([SPACE], dtype=np.uint8))
                joined.append(words[w])
            out = np.concatenate(joined).astype(np.uint8)
    return out[:max_len]


def _pack(titles, stride):
    enc = np.zeros((len(titles), stride), dtype=np.uint8)
    lengths = np.zeros(len(titles), dtype=np.uint8)
    for row, title in enumerate(titles):
        enc[row, :title.shape[0]] = title
        lengths[row] = title.shape[0]
    return enc, lengths


class Case:
    """q_enc uint8[n_q, stride], q_len uint8[n_q]; t_enc, t_len, t_counts uint32[n_t, 15] likewise; t_source[r] = the query
    row truth row r was derived from (-1: none).  q_large / t_large: the title holds a code >= 64."""

    def __init__(self, q_enc, q_len, t_enc, t_len, t_counts, t_source):
        self.q_enc, self.q_len, self.t_enc, self.t_len, self.t_counts, self.t_source = (q_enc, q_len, t_enc, t_len,
                                                                                        t_counts, t_source)
        self.n_q, self.n_t, self.stride = q_enc.shape[0], t_enc.shape[0], q_enc.shape[1]
        inside = lambda enc, lengths: np.arange(enc.shape[1])[None, :] < lengths[:, None]
        self.q_large = ((q_enc >= 64) & inside(q_enc, q_len)).any(axis=1)
        self.t_large = ((t_enc >= 64) & inside(t_enc, t_len)).any(axis=1)
        self.derived = {}
        for row in np.nonzero(t_source >= 0)[0]:
            self.derived.setdefault(int(t_source[row]), []).append(int(row))


def make_case(n_q, n_t, seed, stride=255):
    """Seeded tables of n_q query and n_t truth titles, `stride` bytes per row, lengths up to min(stride, 255).  Both start
    with the edge block (every edge length x style x alphabet); the truth table goes on with the word specials; behind
    them random titles (short ones most often), every third truth row derived from one of the first 6,000 query rows --
    one in five of those with a twin in the next row -- and an (empty, full-length) pair of rows every 50 rows."""
    rng = np.random.RandomState(seed)
    max_len = min(stride, 255)

    def random_title():
        return make_title(rng, _random_length(rng, max_len), STYLES[rng.randint(4)], rng.rand() < 0.15,
                          pool=int(rng.choice((3, 6, 30))))

    queries = _edge_block(rng, max_len)
    while len(queries) < n_q:
        if len(queries) % 50 == 0:
            queries += [np.zeros(0, dtype=np.uint8), make_title(rng, max_len, "words", False)]
        else:
            queries.append(random_title())
    queries = queries[:n_q]
    truth = _edge_block(rng, max_len) + _truth_specials(rng, max_len)
    source = [-1] * len(truth)
    while len(truth) < n_t:
        if len(truth) % 50 == 0:
            truth += [np.zeros(0, dtype=np.uint8), make_title(rng, max_len, "ragged", False)]
            source += [-1, -1]
        elif len(truth) % 3 == 0:
            q = int(rng.randint(min(n_q, 6000)))
            truth.append(_mutate(rng, queries[q], max_len))
            source.append(q)
            if rng.rand() < 0.2:
                truth.append(truth[-1].copy())
                source.append(q)
        else:
            truth.append(random_title())
            source.append(-1)
    truth, source = truth[:n_t], source[:n_t]
    q_enc, q_len = _pack(queries, stride)
    t_enc, t_len = _pack(truth, stride)
    # word counts: 0 (idf = inf), 1, N_TRUTH (idf = 0), above N_TRUTH (idf < 0) and anything between
    menu = np.array([0, 1, N_TRUTH, N_TRUTH + 1, 5 * N_TRUTH], dtype=np.uint32)
    counts = rng.randint(2, N_TRUTH, (n_t, WORDS)).astype(np.uint32)
    special = rng.rand(n_t, WORDS) < 0.4
    counts[special] = menu[rng.randint(0, menu.shape[0], int(special.sum()))]
    counts[::17] = 0                                         # whole rows of zero counts: nanmax = inf, inf - inf
    return Case(q_enc, q_len, t_enc, t_len, counts, np.array(source, dtype=np.int64))


def rows255(enc):
    """Rows padded or cut to the 255 bytes the oracle's callers use."""
    if enc.shape[1] == 255:
        return enc
    out = np.zeros((enc.shape[0], 255), dtype=np.uint8)
    width = min(255, enc.shape[1])
    out[:, :width] = enc[:, :width]
    return out


# ---- candidate rows -------------------------------------------------------------------------------------------------

def make_rows(case, q_first, n_queries, k, seed):
    """int32[n_queries, k]: the candidate truth rows of query rows q_first .. q_first + n_queries.  The recipe changes with
    the query (i % 8) so that the kernel's path changes from one candidate to the next inside a run:
      0  a title with a code >= 64 (literal path), then a short plain one (bit-parallel), alternating;
      1  a plain title, then one with large codes, alternating, both of any length;
      2  an empty truth title, then a 255-character one, alternating;
      3  every truth row twice in a row; query 4 starts with the row query 3 ended on;
      5  random rows, about a third of them outside the table (-1, n_t, INT32_MAX);
      6  the truth rows derived from this query -- all but the first of them twice -- in front of random ones;
      7  random rows, the last of them the rows derived from this query, once each.
    On top: every 37th query is all -1, every 11th has -1 in its first slot, every 13th n_t in its last."""
    rng = np.random.RandomState(seed)
    n_t = case.n_t
    t_len = case.t_len.astype(np.int64)
    max_len = int(t_len.max())
    large = np.nonzero(case.t_large)[0]
    plain = np.nonzero(~case.t_large)[0]
    short_plain = np.nonzero(~case.t_large & (t_len >= 1) & (t_len <= 40))[0]
    empty = np.nonzero(t_len == 0)[0]
    full = np.nonzero(t_len == max_len)[0]
    rows = np.empty((n_queries, k), dtype=np.int32)
    slots = np.arange(k)
    carried = 0
    for i in range(n_queries):
        recipe = i % 8
        if recipe == 0:
            row = np.where(slots % 2 == 0, large[rng.randint(0, large.shape[0], k)],
                           short_plain[rng.randint(0, short_plain.shape[0], k)])
        elif recipe == 1:
            row = np.where(slots % 2 == 0, plain[rng.randint(0, plain.shape[0], k)],
                           large[rng.randint(0, large.shape[0], k)])
        elif recipe == 2:
            row = np.where(slots % 2 == 0, empty[rng.randint(0, empty.shape[0], k)],
                           full[rng.randint(0, full.shape[0], k)])
        elif recipe == 3 or recipe == 4:
            row = np.repeat(rng.randint(0, n_t, (k + 1) // 2 + 1), 2)[:k]
            if recipe == 4:
                row[0] = carried
            carried = int(row[-1])
        elif recipe == 5:
            row = rng.randint(0, n_t, k)
            outside = rng.rand(k) < 0.33
            row[outside] = np.array([-1, n_t, INT32_MAX])[rng.randint(0, 3, int(outside.sum()))]
        elif recipe == 6:
            row = rng.randint(0, n_t, k)
            own = case.derived.get(q_first + i, [])
            doubled = np.array(own + own[1:], dtype=np.int64)[:k]
            row[:doubled.shape[0]] = doubled
        else:
            row = rng.randint(0, n_t, k)
            own = np.array(case.derived.get(q_first + i, []), dtype=np.int64)[:k]
            row[k - own.shape[0]:] = own
        rows[i] = row
    rows[::37] = -1
    rows[5::11, 0] = -1
    rows[7::13, k - 1] = n_t
    return rows


def pairs_of_rows(rows, q_first):
    """(pair_q, pair_t) int64 of the rows form: pair i belongs to query row q_first + i // k."""
    n_queries, k = rows.shape
    return q_first + np.repeat(np.arange(n_queries, dtype=np.int64), k), rows.reshape(-1).astype(np.int64)


def valid_pairs(case, pair_q, pair_t):
    pair_q, pair_t = np.asarray(pair_q, dtype=np.int64), np.asarray(pair_t, dtype=np.int64)
    return (pair_q >= 0) & (pair_q < case.n_q) & (pair_t >= 0) & (pair_t < case.n_t)


def literal_pairs(case, pair_q, pair_t):
    """Per pair, whether the whole-title comparison of construct_features leaves the bit-parallel path, and why:
    (literal, summed length > 255, shorter title > 64 characters, a code >= 64).  False for pairs outside the tables."""
    valid = valid_pairs(case, pair_q, pair_t)
    q = np.where(valid, pair_q, 0).astype(np.int64)
    t = np.where(valid, pair_t, 0).astype(np.int64)
    lq, lt = case.q_len[q].astype(np.int64), case.t_len[t].astype(np.int64)
    too_long = valid & (lq + lt > 255)
    wide_pattern = valid & (np.minimum(lq, lt) > 64)
    big_code = valid & (case.q_large[q] | case.t_large[t])
    return too_long | wide_pattern | big_code, too_long, wide_pattern, big_code


def mixed_runs(flags, valid, k):
    """How many runs of k consecutive pairs hold a valid pair with the flag set directly in front of, or behind, a valid
    pair without it -- the path changes from one candidate to the next while the query stays staged."""
    flags, valid = np.asarray(flags).reshape(-1, k), np.asarray(valid).reshape(-1, k)
    if k < 2:
        return 0
    both = valid[:, 1:] & valid[:, :-1]
    return int((both & (flags[:, 1:] != flags[:, :-1])).any(axis=1).sum())


# ---- expected values ------------------------------------------------------------------------------------------------

def expected_features(oracle, case, pair_q, pair_t, n_truth=N_TRUTH, space=SPACE):
    """uint32[n, 66]: the bits of oracle.construct_features for every pair inside the tables, 0x7fc00000 in all 66 slots
    of a pair outside them."""
    valid = valid_pairs(case, pair_q, pair_t)
    q = np.where(valid, pair_q, 0).astype(np.int64)
    t = np.where(valid, pair_t, 0).astype(np.int64)
    q_enc, t_enc = rows255(case.q_enc), rows255(case.t_enc)
    with np.errstate(all="ignore"):
        bits = oracle.construct_features(case.q_len[q], case.t_len[t], q_enc[q], t_enc[t], case.t_counts[t], space,
                                         n_truth).view(np.uint32).copy()
    bits[~valid] = NAN_BITS
    return bits


def expected_ratios(oracle, case, pair_q, pair_t, threshold, sort_key, space=SPACE):
    """uint8[n]: oracle.close_ratios for every pair inside the tables, 0 for a pair outside them."""
    valid = valid_pairs(case, pair_q, pair_t)
    q = np.where(valid, pair_q, 0).astype(np.int64)
    t = np.where(valid, pair_t, 0).astype(np.int64)
    q_enc, t_enc = rows255(case.q_enc), rows255(case.t_enc)
    ratios = oracle.close_ratios(case.q_len[q], case.t_len[t], q_enc[q], t_enc[t], space, sort_key, threshold)
    ratios[~valid] = 0
    return ratios


# ---- the cases the tests share (sizes and seeds are part of what tests/test_title_cases_cpu.py pins) -----------------

def forms_case():
    """The tables of the launch-form tests: 1,500 queries x 1,200 truth titles."""
    return make_case(1500, 1200, seed=2024)


def forms_queries(k):
    """Queries per rows-form launch: 203 (61 at k >= 100)."""
    return 203 if k < 100 else 61


def forms_rows(case, k, q_first):
    return make_rows(case, q_first, forms_queries(k), k, seed=1000 + k)


GRID_QUERIES, GRID_K = 40000, 16          # 40,000 units of 16 pairs: every wave of the capped grid pops several times


def grid_case():
    return make_case(GRID_QUERIES, 3000, seed=77)


def close_case():
    """The tables of the close-match tests: 6,000 queries x 6,000 truth titles (2,000 of them derived from a query)."""
    return make_case(6000, 6000, seed=78)


def close_queries(k):
    return 500 if k < 100 else 300


def word_counts(enc, lengths, space=SPACE):
    """str.split() word count of every title."""
    inside = np.arange(enc.shape[1])[None, :] < lengths[:, None]
    is_char = (enc != space) & inside
    starts = is_char.copy()
    starts[:, 1:] &= ~is_char[:, :-1]
    return starts.sum(axis=1)


def special_rows(enc, lengths, large, most=48):
    """Rows of a table the close-match kernel treats specially: empty, nothing but spaces, 100 words and more (128 is the
    capacity of its token table), a code >= 64 in a short title (the diagonal DP instead of the bit-parallel LCS)."""
    words = word_counts(enc, lengths)
    lengths = lengths.astype(np.int64)
    empty = np.nonzero(lengths == 0)[0][:4]
    spaces = np.nonzero((lengths > 0) & (words == 0))[0][:12]
    many = np.nonzero(words >= 100)[0][:12]
    coded = np.nonzero(large & (lengths <= 33))[0][:most - 28]
    return np.concatenate((empty, spaces, many, coded)).astype(np.int32)


CLOSE_PASS_QUERIES = 5000                 # x k = 10: 50,000 pairs, past the 32,768 one pass of the close-ratio grid takes
