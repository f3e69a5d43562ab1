#!/usr/bin/env python3
"""Golden vectors of the training objective and of the prediction stages (run in the BUILD container only, on the CPU):

    train_objective.npz  train.py's fast_weighted_log_loss (:32-39) on ~4,000 rows, once on inputs widened to float64 (what
                         numba computes: `beta + actual` with an int64 global promotes the expression) and once on the
                         float32 inputs as NumPy evaluates them, with a per-row flag where the two differ after
                         quantisation to 2^-30; fast_custom_error (:17-29) in both typings and
                         get_evaluation_error_matrix (:63-82, plain NumPy in the reference too) on planted probabilities
                         that hold the float32 nearest to every threshold and both its neighbours, with
                         settings.PREDICTION_PROBABILITY_THRESHOLD at 0.9, 0.5, 0.6 and 0.7, for the whole array and
                         row by row (a call on the one row), with a flag where the typings disagree;
    predict_stages.npz   predict.py's Prediction._get_levenshtein_deletion_ratio / _get_levenshtein_ratio (:140-156) and
                         common.py's two rounded ratios on a few hundred title pairs, and the stage functions
                         _find_exact_matches, _find_close_matches, _find_matches_using_model and _finalize_output
                         (:97-113, :163-183, :185-254, :256-272) on ~60 crafted titles with top_n = 4, at the same four
                         probability thresholds, followed by the counting loop of cli.py:88-132 on the final table;
    predict_end_to_end.npz  the same stage functions at 0.9 with the reference's own MatchMaker (match_maker.py, top_n = 4)
                         in place of the planted candidate lists: 18 titles, each with exactly four truth rows made of its
                         own words, so that no top-4 has a near-tie at its cut; a margin is planted for every candidate
                         MatchMaker gives, and the stand-in model returns its float32 sigmoid;
    predict_two_chunks.npz  generate_test_predictions itself (predict.py:274-321) over the 10,003 titles of
                         tests/chunk_cases.py with top_n = 2: its loop cuts them into chunks of 10,000 and 3.

Everything runs the reference's own function bodies under make_golden.py's shims (numba as pass-through decorators).  The
stage functions are driven on a bare Prediction.__new__(Prediction) object: the truth frame, the candidate lists (a
stand-in match_maker with `top_n` and `get_closest_matches`) and the probabilities (a stand-in model whose `predict`
returns what was planted for the rows of `remaining`) are planted; `construct_features` in the predict module is a no-op
and the mapping_* dicts hold zero rows of the right shape; FINAL_OUTPUT_FILE points into a temporary directory.

Two more stand-ins, in this process only:
  * a module `xgboost` whose DMatrix(a, **kw) returns a;
  * `ratio` inside doppelspeller.common (python-Levenshtein's `ratio`, which is not installed): the published rule,
    (len_a + len_b - indel_distance) / (len_a + len_b), 1.0 for two empty strings, in a few lines of plain Python below.
    THIS ONE FUNCTION IS A STAND-IN; everything that calls it (levenshtein_ratio, levenshtein_token_sort_ratio,
    _get_levenshtein_ratio, the stages) is the reference's.

The fixtures are written with fixed zip timestamps, so a second run reproduces the same bytes.  Nothing is written
under the reference tree.

Usage:  PYTHONHASHSEED=0 python tests/golden/make_golden_predict.py
"""
import io
import logging
import os
import re
import shutil
import sys
import tempfile
import types
import warnings
import zipfile

if os.environ.get("PYTHONHASHSEED") != "0":
    sys.exit("run with PYTHONHASHSEED=0 (the reference's sets and dicts are iterated)")
sys.dont_write_bytecode = True

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import chunk_cases  # noqa: E402
import make_golden  # noqa: E402
import title_cases  # noqa: E402

REFERENCE = make_golden.REFERENCE
THRESHOLDS = (0.9, 0.5, 0.6, 0.7)       # the reference's own first; float32(0.6) > 0.6, float32(0.7) < 0.7
TOP_N = 4
QUANTUM = 2.0 ** 30


def _save(path, **arrays):
    """np.savez_compressed with fixed timestamps (reproducible bytes)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as archive:
        for name, value in arrays.items():
            buffer = io.BytesIO()
            np.lib.format.write_array(buffer, np.asanyarray(value), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            archive.writestr(info, buffer.getvalue())


def _utf8(strings):
    return np.array([s.encode("utf-8") for s in strings])


# ---- the stand-ins ---------------------------------------------------------------------------------------------------

def _lcs(a, b):
    """Length of the longest common subsequence, bit-parallel over Python integers."""
    masks = {}
    for i, character in enumerate(a):
        masks[character] = masks.get(character, 0) | (1 << i)
    full = (1 << len(a)) - 1
    v = full
    for character in b:
        u = v & masks.get(character, 0)
        v = ((v + u) | (v - u)) & full
    return len(a) - bin(v).count("1")


def ratio(a, b):
    """STAND-IN for Levenshtein.ratio: (len_a + len_b - indel_distance) / (len_a + len_b), 1.0 for two empty strings;
    the indel distance (insertions and deletions only) is len_a + len_b - 2 * LCS."""
    total = len(a) + len(b)
    if total == 0:
        return 1.0
    indel_distance = total - 2 * _lcs(a, b)
    return (total - indel_distance) / total


def _lcs_plain(a, b):
    row = [0] * (len(b) + 1)
    for x in a:
        previous = 0
        for j, y in enumerate(b):
            previous, row[j + 1] = row[j + 1], previous + 1 if x == y else max(row[j + 1], row[j])
    return row[len(b)]


def _install_stand_ins():
    make_golden._install_shims()
    xgboost = types.ModuleType("xgboost")
    xgboost.DMatrix = lambda a, **kw: a
    sys.modules["xgboost"] = xgboost
    sys.modules["Levenshtein"].ratio = ratio


# ---- train_objective.npz -----------------------------------------------------------------------------------------------

def _around(value):
    """The float32 nearest to `value` and its two float32 neighbours, ascending."""
    nearest = np.float32(value)
    return [np.nextafter(nearest, np.float32(-np.inf)), nearest, np.nextafter(nearest, np.float32(np.inf))]


class _PlantedModel:
    """Stands in for the booster: predict returns a copy of what was planted (the reference writes into it)."""
    best_ntree_limit = 7

    def __init__(self, planted=None):
        self.planted = planted

    def predict(self, data, ntree_limit=None):
        assert ntree_limit == self.best_ntree_limit
        assert len(data) == len(self.planted)
        return np.array(self.planted, dtype=np.float32)


def _objective(train, s):
    rng = np.random.RandomState(31)
    special = [np.float32(0), np.float32(1), np.float32(1e-45)] + _around(0.5) + _around(0.9) + _around(1.0)
    p = np.concatenate((np.array(special, dtype=np.float32), rng.rand(2000 - len(special)).astype(np.float32)))
    p = np.concatenate((p, p))                                                   # every probability with both labels
    y = np.repeat(np.array([0, 1], dtype=np.float32), p.shape[0] // 2)
    with np.errstate(all="ignore"):
        g64, h64 = train.fast_weighted_log_loss(p.astype(np.float64), y.astype(np.float64))
        g32, h32 = train.fast_weighted_log_loss(p, y)
    assert g64.dtype == np.float64 and h64.dtype == np.float64 and g32.dtype == np.float32 and h32.dtype == np.float32
    quantised = lambda x: np.rint(np.asarray(x, dtype=np.float64) * QUANTUM)
    typing_differs = (quantised(g64) != quantised(g32)) | (quantised(h64) != quantised(h32))

    # fast_custom_error and get_evaluation_error_matrix
    planted = [np.float32(0), np.float32(1)]
    for threshold in THRESHOLDS:
        planted += _around(threshold)
    q = np.concatenate((np.array(planted, dtype=np.float32), rng.rand(330).astype(np.float32)))
    q = np.concatenate((q, q))
    t = np.repeat(np.array([0, 1], dtype=np.float32), q.shape[0] // 2)
    order = rng.permutation(q.shape[0])
    q, t = q[order], t[order]
    n = q.shape[0]
    error64, error32 = np.zeros(len(THRESHOLDS), np.int64), np.zeros(len(THRESHOLDS), np.int64)
    matrix = np.zeros((len(THRESHOLDS), 4), np.int64)
    positive64, positive32, positive_matrix = (np.zeros((len(THRESHOLDS), n), dtype=bool) for _ in range(3))
    own = s.PREDICTION_PROBABILITY_THRESHOLD
    assert own == THRESHOLDS[0]

    def positive_of(cost, label):       # one row's cost -> was it predicted positive (a false negative costs 1, a false
        return cost == 0 if label else cost != 0                                        # positive the penalty factor)

    for i, threshold in enumerate(THRESHOLDS):
        s.PREDICTION_PROBABILITY_THRESHOLD = threshold
        error64[i] = train.fast_custom_error(q.astype(np.float64), t)
        error32[i] = train.fast_custom_error(q, t)
        matrix[i] = train.get_evaluation_error_matrix(_PlantedModel(q), q, t)
        for row in range(n):
            one_q, one_t = q[row:row + 1], t[row:row + 1]
            positive64[i, row] = positive_of(train.fast_custom_error(one_q.astype(np.float64), one_t), t[row])
            positive32[i, row] = positive_of(train.fast_custom_error(one_q, one_t), t[row])
            tp, tn, fp, fn = train.get_evaluation_error_matrix(_PlantedModel(one_q), one_q, one_t)
            assert tp + tn + fp + fn == 1
            positive_matrix[i, row] = bool(tp + fp)
    s.PREDICTION_PROBABILITY_THRESHOLD = own
    typings_disagree = positive64 != positive32
    assert np.array_equal(positive32, positive_matrix)
    _save(f"{HERE}/train_objective.npz",
          p=p, y=y, g64=g64, h64=h64, g32=g32, h32=h32, typing_differs=typing_differs,
          beta=np.int64(s.FALSE_POSITIVE_PENALTY_FACTOR), thresholds=np.array(THRESHOLDS, dtype=np.float64),
          planted_p=q, planted_y=t, custom_error_f64=error64, custom_error_f32=error32, error_matrix=matrix,
          positive_f64=positive64, positive_f32=positive32, positive_matrix=positive_matrix,
          typings_disagree=typings_disagree)
    return p.shape[0], int(typing_differs.sum()), n, typings_disagree.sum(axis=1).tolist()


# ---- predict_stages.npz: titles ----------------------------------------------------------------------------------------

WORDS = ("alpha", "beta", "gamma", "delta", "omega", "limited", "holdings", "services", "trading", "partners", "group",
         "north", "south", "capital", "systems", "global", "bv", "ltd", "co", "a1", "zz9", "mn", "pq", "x", "q7",
         "ventures", "logistics", "motors", "foods", "digital", "marine", "energy", "studio", "labs", "works")
LETTERS = "abcdefghijklmnopqrstuvwxyz0123456789"


class _Titles:
    """Seeded titles and near copies of them, the reference's own _get_levenshtein_ratio deciding what is near."""

    def __init__(self, prediction_class, seed):
        self.rng = np.random.RandomState(seed)
        self.ratio_of = prediction_class._get_levenshtein_ratio
        self.used = set()

    def fresh(self, n_words=None, length=None, min_length=3):
        """A title nobody has: n_words words (min_length characters at least), or exactly `length` characters."""
        while True:
            if length is None:
                title = " ".join(self.rng.choice(WORDS, n_words or self.rng.randint(3, 6)))
            else:
                title = " ".join(self.rng.choice(WORDS, length))[:length].rstrip()
                title += "".join(self.rng.choice(list(LETTERS), length - len(title)))
            if title not in self.used and len(title) >= min_length:
                self.used.add(title)
                return title

    def edited(self, title, edits):
        out = list(title)
        for _ in range(edits):
            at = int(self.rng.randint(len(out)))
            how = int(self.rng.randint(3))
            if how == 0 and len(out) > 3 and out[at] != " ":
                del out[at]
            elif how == 1 and len(out) < 255:
                out.insert(at, str(self.rng.choice(list(LETTERS))))
            elif out[at] != " ":
                out[at] = str(self.rng.choice(list(LETTERS)))
        return " ".join("".join(out).split())

    def near(self, title, wanted, shuffle=False):
        """A title nobody has whose ratio to `title` (predict.py:147-156) is `wanted`; shuffle: its words in another
        order first, so that only the token-sort ratio can be high."""
        for attempt in range(20000):
            base = title
            if shuffle:
                words = title.split()
                base = " ".join(words[1:] + words[:1]) if attempt % 2 else " ".join(words[::-1])
            other = self.edited(base, attempt % 7)
            if other != title and other not in self.used and len(other) >= 3 and self.ratio_of(title, other) == wanted:
                self.used.add(other)
                return other
        raise AssertionError(f"no title at ratio {wanted} of {title!r}")


def _ratio_pairs(common, prediction_class, alphabet):
    """The (x, y) pairs of the ratio section."""
    rng = np.random.RandomState(94)
    titles = _Titles(prediction_class, 95)
    pairs = [("a", "a"), ("a", "b"), ("a", "ab"), ("ab", "a"), ("abc", "abc"), ("abc", "abd"), ("abc", "acb"),
             ("abc", "ab c"), ("a b", "b a"), ("abc", "bca"), ("x", "x" * 255), ("x" * 255, "x")]

    def of_length(n):
        return titles.fresh(length=n)

    # length pairs on both sides of the pre-filter's 94 (and where it is 94 exactly): y a prefix of x, or x a prefix of y
    for lx, ly in ((53, 47), (47, 53), (106, 94), (159, 141), (50, 44), (50, 45), (44, 50), (45, 50), (100, 88), (100, 89),
                   (255, 225), (255, 226), (255, 227), (226, 255), (227, 255), (17, 15), (16, 15), (33, 29), (33, 30),
                   (3, 4), (4, 3), (3, 3), (255, 255), (255, 254), (254, 255), (255, 240), (240, 255)):
        long_one = of_length(max(lx, ly))
        short_one = long_one[:min(lx, ly)]
        if short_one.endswith(" "):
            short_one = short_one[:-1] + "k"
        pairs.append((long_one, short_one) if lx >= ly else (short_one, long_one))
        assert (len(pairs[-1][0]), len(pairs[-1][1])) == (lx, ly)
    # plain ratios of exactly 94 and 95, and their neighbours, at several lengths
    for n_words in (2, 3, 4, 5, 6, 8, 12):
        for wanted in (93, 94, 95, 96):
            x = titles.fresh(n_words=n_words)
            try:
                pairs.append((x, titles.near(x, wanted) if wanted > 94 else _plain_at(titles, common, x, wanted)))
            except AssertionError:              # no such ratio at this length
                pass
    # pairs that only the token-sort ratio lifts above 94
    for n_words in (2, 3, 4, 5, 7, 10):
        for wanted in (95, 97, 100):
            x = titles.fresh(n_words=n_words)
            try:
                y = titles.near(x, wanted, shuffle=True)
            except AssertionError:              # no such ratio at this length
                continue
            if common.levenshtein_ratio(x, y) <= 94:
                pairs.append((x, y))
    # 255 characters: one substitution, words in another order
    x = of_length(255)
    pairs += [(x, x), (x, x[:100] + ("q" if x[100] != "q" else "r") + x[101:]), (x, " ".join(x.split()[::-1]))]
    # the hostile titles of tests/title_cases.py that are text (codes below 64), and near copies of them
    decode = lambda codes: "".join(alphabet[c] for c in codes)
    for i in range(220):
        style = title_cases.STYLES[i % 4]
        length = int(rng.choice((1, 2, 3, 4, 8, 17, 31, 32, 33, 50, 63, 64, 65, 100, 127, 128, 129, 200, 253, 254, 255)))
        x = title_cases.make_title(rng, length, style, False, pool=int(rng.choice((3, 6, 30))))
        y = title_cases._mutate(rng, x, 255)
        if x.shape[0] + y.shape[0] > 0 and y.shape[0] > 0:
            pairs.append((decode(x), decode(y)))
    return pairs


def _plain_at(titles, common, title, wanted, both=False):
    """A title nobody has whose PLAIN rounded ratio to `title` is `wanted` (<= 94: _get_levenshtein_ratio falls back to
    the token-sort ratio, which an edit may move); both: _get_levenshtein_ratio gives `wanted` as well."""
    for attempt in range(20000):
        other = titles.edited(title, 1 + attempt % 4)
        if other != title and other not in titles.used and len(other) >= 3 and \
                common.levenshtein_ratio(title, other) == wanted and \
                (not both or titles.ratio_of(title, other) == wanted):
            titles.used.add(other)
            return other
    raise AssertionError(f"no title at plain ratio {wanted} of {title!r}")


# ---- predict_stages.npz: the stage cases -------------------------------------------------------------------------------

class _Cases:
    """The truth rows, the titles, their TOP_N candidate rows and planted probabilities, and a planted actual id."""

    def __init__(self, prediction_class, common):
        self.titles_of = _Titles(prediction_class, 7)
        self.common = common
        self.truth, self.title, self.rows, self.p, self.actual, self.name = [], [], [], [], [], []
        self.low = iter(np.linspace(0.01, 0.45, 400).astype(np.float32))      # distinct low probabilities
        self.decoys = [self.add_truth(self.titles_of.fresh()) for _ in range(10)]
        self.decoy_at = 0

    def add_truth(self, title):
        self.truth.append(title)
        return len(self.truth) - 1

    def decoy(self):
        self.decoy_at += 1
        return self.decoys[self.decoy_at % len(self.decoys)]

    def add(self, name, title, rows, p, actual):
        """rows / p: None stands for a decoy row / a low probability of its own.  actual: a slot, -1 (no match to find),
        "other" (an id no truth row has) or ("row", r)."""
        rows = [self.decoy() if r is None else r for r in rows]
        p = [next(self.low) if v is None else np.float32(v) for v in p]
        assert len(rows) == TOP_N and len(p) == TOP_N
        self.title.append(title)
        self.rows.append(rows)
        self.p.append(p)
        if isinstance(actual, tuple):
            self.actual.append(actual[1])
        else:
            self.actual.append(-1 if actual == -1 else (-2 if actual == "other" else rows[actual]))
        self.name.append(name)

    def near_row(self, title, wanted, shuffle=False):
        return self.add_truth(self.titles_of.near(title, wanted, shuffle=shuffle))

    def plain_row(self, title, wanted):
        return self.add_truth(_plain_at(self.titles_of, self.common, title, wanted, both=True))


def _stage_cases(prediction_class, common):
    c = _Cases(prediction_class, common)
    fresh = lambda **how: c.titles_of.fresh(min_length=32, **how)    # long enough for every ratio from 93 to 99
    N = None
    up = lambda t: _around(t)[2]
    at = lambda t: _around(t)[1]
    down = lambda t: _around(t)[0]

    # exact: a truth title held by two and by three rows (the last id wins), and by one
    for copies in (2, 3, 1, 2, 3, 1):
        title = fresh()
        rows = [c.add_truth(title) for _ in range(copies)]
        c.add_truth(fresh())
        # the candidates hold an earlier copy with a high probability: the exact stage answers first all the same
        c.add(f"exact_{copies}", title, [rows[0], N, N, N], [0.99, N, N, N], ("row", rows[-1 if copies < 3 else 0]))
    # close: a single candidate above 94
    for slot, wanted in enumerate((95, 96, 97, 98, 99)):
        title = fresh(n_words=5 + slot)
        rows = [N] * TOP_N
        rows[slot % TOP_N] = c.near_row(title, wanted)
        c.add(f"close_single_{wanted}", title, rows, [N] * TOP_N, slot % TOP_N if slot != 2 else -1)
    for length in (255, 254):
        title = fresh(length=length)
        c.add(f"close_long_{length}", title, [N, c.near_row(title, 99), N, N], [N] * TOP_N, 1)
    # close: two above 94, the higher one wins wherever it stands
    for slots in ((0, 3), (3, 0), (1, 2)):
        title = fresh(n_words=6)
        rows = [N] * TOP_N
        rows[slots[0]], rows[slots[1]] = c.near_row(title, 95), c.near_row(title, 97)
        c.add("close_two_above", title, rows, [N] * TOP_N, slots[1])
    # close: two tied at the maximum: no close match, the title goes on to the model
    title = fresh(n_words=6)
    c.add("close_tie_then_model", title, [c.near_row(title, 97), c.near_row(title, 97), c.near_row(title, 95), N],
          [N, N, 0.95, N], 2)
    title = fresh(n_words=6)
    c.add("close_tie_then_none", title, [c.near_row(title, 96), N, N, c.near_row(title, 96)], [0.5, N, N, 0.6], 0)
    title = fresh(n_words=6)
    c.add("close_tie_then_model_tie", title, [c.near_row(title, 98), N, c.near_row(title, 98), N],
          [0.97, N, 0.97, N], -1)
    # close: a maximum of exactly 94 is no close match
    title = fresh(n_words=6)
    c.add("close_94_then_model", title, [N, c.plain_row(title, 94), N, N], [N, 0.97, N, N], 1)
    title = fresh(n_words=6)
    c.add("close_94_then_none", title, [c.plain_row(title, 94), N, N, N], [0.7, N, N, N], 0)
    title = fresh(n_words=6)
    c.add("close_94_and_95", title, [c.plain_row(title, 94), N, c.near_row(title, 95), N], [0.99, N, N, N], 2)
    # close: only the token-sort ratio is above 94
    for wanted in (95, 97, 100):
        while True:
            title = fresh(n_words=5)
            if len(set(title.split())) < 5:
                continue
            try:
                row = c.near_row(title, wanted, shuffle=True)
                break
            except AssertionError:          # no such ratio at this length
                pass
        assert common.levenshtein_ratio(title, c.truth[row]) <= 94
        c.add(f"close_token_sort_{wanted}", title, [N, N, row, N], [N] * TOP_N, 2 if wanted != 97 else "other")
    while True:
        title = fresh(n_words=4)
        if len(set(title.split())) == 4:
            break
    words = title.split()
    c.add("close_token_sort_tie", title, [c.add_truth(" ".join(words[::-1])), c.add_truth(" ".join(words[1:] + words[:1])),
                                          N, N], [0.3, 0.93, N, N], 1)
    # close: the pre-filter zeroes a candidate that is a prefix of the title
    for length, kept in ((50, 44), (100, 88)):
        title = fresh(length=length)
        prefix = title[:kept].rstrip()
        prefix += "k" * (kept - len(prefix))
        c.add("close_prefilter", title, [c.add_truth(prefix), N, N, N], [0.92, N, N, N], 0)
    # model: the maximum at the float32 nearest to each threshold, at its upper and at its lower neighbour
    for threshold in THRESHOLDS:
        for name, value in (("at", at(threshold)), ("up", up(threshold)), ("down", down(threshold))):
            slot = len(c.title) % TOP_N
            p = [N] * TOP_N
            p[slot] = value
            c.add(f"model_{name}_{threshold}", fresh(), [N] * TOP_N, p, slot if name != "down" else -1)
    # model: ties at the maximum, a tie below it
    c.add("model_tie_2", fresh(), [N] * TOP_N, [0.97, N, 0.97, N], 0)
    c.add("model_tie_3", fresh(), [N] * TOP_N, [N, 0.99, 0.99, 0.99], -1)
    c.add("model_tie_below_the_maximum", fresh(), [N] * TOP_N, [0.55, 0.55, N, 0.95], 3)
    c.add("model_tie_at_one", fresh(), [N] * TOP_N, [1.0, N, N, 1.0], 3)
    # the same truth id twice among a title's candidates
    row = c.decoy()
    c.add("twice_single_maximum", fresh(), [row, N, row, N], [0.95, N, 0.3, N], 0)
    row = c.decoy()
    c.add("twice_tied_maximum", fresh(), [N, row, row, N], [N, 0.96, 0.96, N], 1)
    title = fresh(n_words=6)
    row = c.near_row(title, 97)
    c.add("twice_close_tie", title, [row, row, N, N], [N, N, 0.95, N], 0)
    # model: a single maximum well above, and nothing at all
    for slot, value in enumerate((0.99, 1.0, 0.91, 0.999)):
        p = [N] * TOP_N
        p[slot] = value
        c.add("model_single", fresh(), [N] * TOP_N, p, slot if slot != 1 else "other")
    for actual in (-1, -1, 2):
        c.add("none", fresh(), [N] * TOP_N, [N] * TOP_N, actual)
    return c


class _MatchMaker:
    """Stands in for MatchMaker: the planted candidate ids of a row."""

    def __init__(self, candidate_ids):
        self.top_n, self.candidate_ids = candidate_ids.shape[1], candidate_ids

    def get_closest_matches(self, row_number):
        return [int(v) for v in self.candidate_ids[row_number]]


def _run_stages(predict, cli, c, s, truth_titles, truth_ids, titles, match_maker, plant, actual_ids, threshold,
                directory):
    """The reference's four stage functions in the order of generate_test_predictions (predict.py:288-319), one chunk.
    match_maker: what stands at Prediction.match_maker; plant(test indexes, match title ids) -> the probabilities the
    stand-in model returns for the rows of `remaining`."""
    import pandas as pd
    n = len(titles)
    s.PREDICTION_PROBABILITY_THRESHOLD = threshold
    s.FINAL_OUTPUT_FILE = f"{directory}/final_output.csv"
    s.TEST_WITH_ACTUALS_FILE = f"{directory}/test_with_actuals.csv"
    truth_data = pd.DataFrame({c.COLUMN_TITLE_ID: truth_ids, c.COLUMN_TRANSFORMED_TITLE: truth_titles})
    data = pd.DataFrame({c.COLUMN_TEST_INDEX: np.arange(n), c.COLUMN_TRANSFORMED_TITLE: titles})
    model = _PlantedModel()
    p = predict.Prediction.__new__(predict.Prediction)
    p.fe = types.SimpleNamespace(data=data, truth_data=truth_data, space_code=np.uint8(1),
                                 number_of_truth_titles=np.uint32(len(truth_titles)))
    p.test_indexes = list(data[c.COLUMN_TEST_INDEX])
    p.model = model
    p.match_maker = match_maker
    p.matched_so_far = []
    p.predictions_columns = [c.COLUMN_TEST_INDEX, c.COLUMN_TRANSFORMED_TITLE, c.COLUMN_MATCH_TRANSFORMED_TITLE,
                             c.COLUMN_MATCH_TITLE_ID, c.COLUMN_PREDICTION]
    p.predictions = pd.DataFrame(index=[], columns=p.predictions_columns)
    p.truth_data_mapping, p.truth_data_mapping_reversed = p._get_truth_data_mappings(truth_data)
    p.mapping_title_encoding = {i: np.zeros(255, dtype=np.uint8) for i in range(n)}
    p.mapping_truth_title_encoding = {int(i): np.zeros(255, dtype=np.uint8) for i in truth_ids}
    p.mapping_truth_words_counts = {int(i): np.zeros(15, dtype=np.uint32) for i in truth_ids}

    p._find_exact_matches()
    after_exact = list(p.matched_so_far)
    chunk = p.fe.data.loc[:, [c.COLUMN_TEST_INDEX, c.COLUMN_TRANSFORMED_TITLE]].copy(deep=True)      # :295-296
    chunk.loc[:, c.COLUMN_TEST_INDEX] = chunk[c.COLUMN_TEST_INDEX].astype(np.uint32)
    p.data = chunk
    remaining = p._find_close_matches()
    after_close = list(p.matched_so_far)
    remaining_q = np.asarray(remaining[c.COLUMN_TEST_INDEX], dtype=np.int64)
    remaining_id = np.asarray(remaining[c.COLUMN_MATCH_TITLE_ID], dtype=np.int64)
    remaining_ratio = np.asarray(remaining[c.COLUMN_LEVENSHTEIN_RATIO], dtype=np.int64)
    assert remaining_q.shape[0] % TOP_N == 0 and (remaining_q.reshape(-1, TOP_N) == remaining_q[::TOP_N, None]).all()
    model.planted = plant(remaining_q, remaining_id)
    p._find_matches_using_model(remaining)
    after_model = list(p.matched_so_far)
    p._finalize_output()
    final = pd.read_csv(s.FINAL_OUTPUT_FILE, sep=s.TEST_FILE_DELIMITER)
    saved = p.predictions
    pd.DataFrame({c.COLUMN_TEST_INDEX: np.arange(n), "name": titles, s.TEST_WITH_ACTUALS_TITLE_ID: actual_ids}).to_csv(
        s.TEST_WITH_ACTUALS_FILE, index=False, sep=s.TEST_FILE_DELIMITER)
    records = []
    handler = logging.Handler()
    handler.emit = lambda record: records.append(record.getMessage())
    cli.LOGGER.addHandler(handler)
    level = cli.LOGGER.level
    cli.LOGGER.setLevel(logging.INFO)
    try:
        assert cli.get_predictions_accuracy.callback() is True
    finally:
        cli.LOGGER.removeHandler(handler)
        cli.LOGGER.setLevel(level)
    report = [r for r in records if "Correctly matched titles" in r]
    assert len(report) == 1
    counts = [int(re.search(label + r"\s+(-?\d+)", report[0]).group(1)) for label in
              ("Correctly matched titles", "Incorrectly matched titles", "Correctly marked as not-found",
               "Incorrectly marked as not-found", "Custom Error")]
    return dict(after_exact=np.array(after_exact, dtype=np.int64), after_close=np.array(after_close, dtype=np.int64),
                after_model=np.array(after_model, dtype=np.int64), remaining_q=remaining_q, remaining_id=remaining_id,
                remaining_ratio=remaining_ratio,
                saved_index=np.asarray(saved[c.COLUMN_TEST_INDEX], dtype=np.int64),
                saved_id=np.asarray(saved[c.COLUMN_MATCH_TITLE_ID], dtype=np.int64),
                saved_prediction=np.asarray(saved[c.COLUMN_PREDICTION], dtype=np.float32),
                final_id=np.asarray(final[c.COLUMN_TITLE_ID], dtype=np.int64),
                final_index=np.asarray(final[c.COLUMN_TEST_INDEX], dtype=np.int64),
                counts=np.array(counts, dtype=np.int64))


def _stages(predict, common, cli, c, s, directory):
    prediction_class = predict.Prediction
    alphabet = f"{s.R_FILL_CHARACTER} abcdefghijklmnopqrstuvwxyz0123456789"
    for a, b in (("kitten", "sitting"), ("", "abc"), ("abcabc", "cab"), ("a b c", "c b a"), ("x" * 70, "x" * 69 + "y")):
        assert _lcs(a, b) == _lcs_plain(a, b)

    # ---- the ratio functions on title pairs
    pairs = [(x, y) for x, y in _ratio_pairs(common, prediction_class, alphabet) if len(x) + len(y) > 0]
    assert all(_lcs(x, y) == _lcs_plain(x, y) for x, y in pairs[::9])
    deletion = np.array([prediction_class._get_levenshtein_deletion_ratio(x, y) for x, y in pairs], dtype=np.float64)
    value = np.array([prediction_class._get_levenshtein_ratio(x, y) for x, y in pairs], dtype=np.int64)
    plain = np.array([common.levenshtein_ratio(x, y) for x, y in pairs], dtype=np.int64)
    token_sort = np.array([common.levenshtein_token_sort_ratio(x, y) for x, y in pairs], dtype=np.int64)
    assert (deletion == 94).any() and (deletion < 94).sum() >= 10 and (plain == 94).sum() >= 4 and (plain == 95).sum() >= 4
    assert ((plain <= 94) & (token_sort > 94) & (value > 94)).sum() >= 8
    lengths = {len(t) for pair in pairs for t in pair}
    assert {1, 3, 255} <= lengths

    # ---- the stage functions
    cases = _stage_cases(prediction_class, common)
    rng = np.random.RandomState(5)
    n_truth, n = len(cases.truth), len(cases.title)
    assert len(set(cases.title)) == n
    truth_ids = (1000 + 7 * rng.permutation(n_truth)).astype(np.int64)           # unique, in no order
    rows = np.array(cases.rows, dtype=np.int32)
    planted = np.array(cases.p, dtype=np.float32)
    candidate_ids = truth_ids[rows]
    spare = int(truth_ids.max()) + 7                                             # an id no truth row has
    actual_ids = np.array([-1 if a == -1 else (spare if a == -2 else truth_ids[a]) for a in cases.actual], dtype=np.int64)
    ratios = np.array([[prediction_class._get_levenshtein_ratio(cases.title[q], cases.truth[t]) for t in rows[q]]
                       for q in range(n)], dtype=np.int64)
    outputs = {}
    for i, threshold in enumerate(THRESHOLDS):
        out = _run_stages(predict, cli, c, s, cases.truth, truth_ids, cases.title, _MatchMaker(candidate_ids),
                          lambda q, _: planted[q, np.arange(q.shape[0]) % TOP_N], actual_ids, threshold, directory)
        for name in ("after_exact", "after_close", "remaining_q", "remaining_id", "remaining_ratio"):
            if i:
                assert np.array_equal(out[name], outputs[name]), name                # no threshold in front of the model
            else:
                outputs[name] = out[name]
        for name in ("after_model", "saved_index", "saved_id", "saved_prediction", "final_id", "final_index", "counts"):
            outputs[f"{name}_{i}"] = out[name]
    s.PREDICTION_PROBABILITY_THRESHOLD = THRESHOLDS[0]
    at_own = outputs["counts_0"]
    assert (at_own[:4] > 0).all(), at_own
    assert (outputs["final_id_0"] == -1).any() and set(outputs["final_index_0"].tolist()) == set(range(n))
    _save(f"{HERE}/predict_stages.npz",
          pair_x=_utf8([x for x, _ in pairs]), pair_y=_utf8([y for _, y in pairs]), pair_deletion_ratio=deletion,
          pair_ratio=value, pair_plain_ratio=plain, pair_token_sort_ratio=token_sort,
          levenshtein_threshold=np.int64(s.LEVENSHTEIN_RATIO_THRESHOLD),
          not_found=np.int64(s.TRAIN_NOT_FOUND_VALUE), thresholds=np.array(THRESHOLDS, dtype=np.float64),
          top_n=np.int64(TOP_N), truth_titles=_utf8(cases.truth), truth_ids=truth_ids, titles=_utf8(cases.title),
          names=_utf8(cases.name), candidate_rows=rows, candidate_ids=candidate_ids, probabilities=planted,
          actual_ids=actual_ids, candidate_ratios=ratios, **outputs)
    return len(pairs), n, n_truth, {t: outputs[f"counts_{i}"].tolist() for i, t in enumerate(THRESHOLDS)}


# ---- predict_end_to_end.npz: the stages behind the reference's own MatchMaker ------------------------------------------

MARGIN_HIGH, MARGIN_BELOW, MARGIN_COPY, MARGIN_DEFAULT = 3.0, 2.0, -5.0, -6.0   # sigmoid 0.953, 0.881, 0.0067, 0.0025


def _probability(margin):
    return np.float32(1) / (np.float32(1) + np.exp(-np.float32(margin), dtype=np.float32))


class _Families:
    """Titles whose Jaccard top-4 is not in doubt: every title has exactly four truth rows made of its own words (near
    copies, copies, or cousins that keep three of its five words); every word is random letters and used by one family
    only.  Title lengths are all different, and so are the lengths of a title's distinct candidates: a model can tell
    every (title, candidate) pair by the two length features and give it the margin planted here."""

    def __init__(self, prediction_class, common):
        self.rng = np.random.RandomState(77)
        self.ratio_of, self.common = prediction_class._get_levenshtein_ratio, common
        self.words, self.title_lengths = set(), set()
        self.truth, self.title, self.family, self.margin, self.name = [], [], [], [], []

    def word(self):
        for _ in range(1000):
            out = "".join(self.rng.choice(list(LETTERS[:26]), self.rng.randint(4, 13)))
            if out not in self.words:
                self.words.add(out)
                return out
        raise RuntimeError("no unused word")

    def new_title(self):
        for _ in range(1000):                                         # 5 words of 4..12 letters: 33 lengths from 32 to 64
            title = " ".join(self.word() for _ in range(5))
            if len(title) not in self.title_lengths and len(title) >= 32:
                self.title_lengths.add(len(title))
                return title
        raise RuntimeError("no unused title length")

    def candidate(self, title, kind, taken):
        """kind: "copy", "cousin", ("near", ratio), ("plain", ratio) or "shuffled"; taken: the lengths in use."""
        if kind == "copy":
            return title
        words = title.split()
        for attempt in range(5000):
            if kind == "cousin":
                keep = sorted(self.rng.choice(5, 3, replace=False).tolist())
                other = " ".join(words[i] if i in keep else self.word() for i in range(5))
                good = self.ratio_of(title, other) < 90
            elif kind == "shuffled":
                other = " ".join(words[i] for i in self.rng.permutation(5))
                good = self.common.levenshtein_ratio(title, other) <= 94 and self.ratio_of(title, other) == 100
            else:
                out = list(title)
                for _ in range(1 + attempt % 4):
                    at = int(self.rng.randint(len(out)))
                    how = int(self.rng.randint(3))
                    if how == 0 and out[at] != " ":
                        del out[at]
                    elif how == 1:
                        out.insert(at, str(self.rng.choice(list(LETTERS[:26]))))
                    elif out[at] != " ":
                        out[at] = str(self.rng.choice(list(LETTERS[:26])))
                other = "".join(out)
                good = " ".join(other.split()) == other and other != title and self.ratio_of(title, other) == kind[1] and \
                    (kind[0] == "near" or self.common.levenshtein_ratio(title, other) == kind[1])
            if good and len(other) not in taken:
                return other
        raise AssertionError(f"no {kind} of {title!r}")

    def add(self, name, kinds, margins):
        """One title and its four truth rows; margins: per row the planted margin, None for a low one of its own (a copy
        of the title has MARGIN_COPY: the exact stage answers before the model is asked)."""
        for _ in range(30):
            title = self.new_title()
            try:
                taken, rows = ({len(title)} if "copy" in kinds else set()), []
                for kind in kinds:
                    other = self.candidate(title, kind, taken)
                    taken.add(len(other))
                    rows.append(other)
                break
            except AssertionError:                  # no such ratio at this length: another title
                self.title_lengths.discard(len(title))
        else:
            raise RuntimeError(name)
        first = len(self.truth)
        self.truth += rows
        self.title.append(title)
        self.family.append(list(range(first, first + 4)))
        self.margin.append([MARGIN_COPY if kind == "copy" else (-3.0 - 0.25 * j if m is None else m)
                            for j, (kind, m) in enumerate(zip(kinds, margins))])
        self.name.append(name)


def _family_cases(prediction_class, common):
    f = _Families(prediction_class, common)
    N, H, B = None, MARGIN_HIGH, MARGIN_BELOW
    near = lambda wanted: ("near", wanted)
    f.add("exact_2", ["cousin", "copy", "cousin", "copy"], [H, N, N, N])
    f.add("exact_3", ["copy", "copy", "cousin", "copy"], [N, N, H, N])
    f.add("exact_1", ["cousin", "cousin", "copy", "cousin"], [H, N, N, N])
    f.add("close_single", [near(97), "cousin", "cousin", "cousin"], [N, H, N, N])
    f.add("close_single", ["cousin", "cousin", "cousin", near(95)], [N, N, N, N])
    f.add("close_two_above", ["cousin", near(95), near(98), "cousin"], [N, H, N, N])
    f.add("close_tie_then_model", [near(97), near(97), "cousin", "cousin"], [N, N, H, N])
    f.add("close_tie_then_none", [near(96), "cousin", near(96), "cousin"], [B, N, N, N])
    f.add("close_94_then_model", ["cousin", ("plain", 94), "cousin", "cousin"], [N, H, N, N])
    f.add("close_94_then_none", [("plain", 94), "cousin", "cousin", "cousin"], [B, N, N, N])
    f.add("close_token_sort", ["cousin", "cousin", "shuffled", "cousin"], [H, N, N, N])
    f.add("model_single", ["cousin"] * 4, [N, N, H, N])
    f.add("model_single", ["cousin"] * 4, [H, B, N, N])
    f.add("model_tie", ["cousin"] * 4, [H, N, N, H])
    f.add("model_below", ["cousin"] * 4, [N, B, N, N])
    f.add("model_tie_below_the_maximum", ["cousin"] * 4, [B, B, N, H])
    f.add("none", ["cousin"] * 4, [N, N, N, N])
    f.add("none", ["cousin"] * 4, [N, N, N, N])
    return f


def _end_to_end(predict, common, match_maker, cli, c, s, directory):
    """The stage functions with the reference's own MatchMaker (top_n = 4) in place of planted candidate lists: the
    candidates of every title are what get_closest_matches gives, and a probability is planted for exactly those."""
    f = _family_cases(predict.Prediction, common)
    rng = np.random.RandomState(9)
    order = rng.permutation(len(f.truth)).tolist()              # the truth rows in no order
    truth = [f.truth[r] for r in order]
    row_of = {int(r): i for i, r in enumerate(order)}
    truth_ids = (500 + 3 * rng.permutation(len(truth))).astype(np.int64)
    n = len(f.title)
    with open(s.GROUND_TRUTH_FILE, "w") as handle:
        handle.write("company_id|name\n" + "".join(f"{i}|{t}\n" for i, t in zip(truth_ids, truth)))
    with open(s.TEST_FILE, "w") as handle:
        handle.write("test_index|name\n" + "".join(f"{i}|{t}\n" for i, t in enumerate(f.title)))
    truth_data, data = common.get_ground_truth(), common.get_test_data()
    assert list(truth_data[c.COLUMN_TRANSFORMED_TITLE]) == truth and list(data[c.COLUMN_TRANSFORMED_TITLE]) == f.title
    mm = match_maker.MatchMaker(data.copy(), truth_data.copy(), TOP_N)
    candidate_ids = np.array([mm.get_closest_matches(q) for q in range(n)], dtype=np.int64)
    id_row = {int(i): row for row, i in enumerate(truth_ids)}
    margins = np.zeros((n, TOP_N), dtype=np.float32)
    planted = {}
    gap = np.zeros(n)
    for q in range(n):
        family = {row_of[r]: m for r, m in zip(f.family[q], f.margin[q])}
        got = [id_row[int(i)] for i in candidate_ids[q]]
        assert sorted(got) == sorted(family), (f.name[q], got, family)       # the four rows of its own words, no other
        for slot, row in enumerate(got):
            margins[q, slot] = family[row]
            planted[(q, int(truth_ids[row]))] = _probability(family[row])
        q_maxint = float(sum([mm._get_idf_given_index(r) for r in mm.matrix_non_zero_columns[q]]))
        jaccard = np.sort(match_maker.fast_jaccard(mm.number_of_truth_titles, q_maxint, mm.matrix_non_zero_columns[q],
                                                   mm.matrix_truth_non_zero_columns_and_values, mm.sums_matrix_truth))[::-1]
        gap[q] = jaccard[TOP_N - 1] - jaccard[TOP_N]
    assert gap.min() > 0.1, gap.min()                                        # no near-tie at the cut of the top 4
    out = _run_stages(predict, cli, c, s, truth, truth_ids, f.title, mm,
                      lambda qs, ids: np.array([planted[(int(q), int(i))] for q, i in zip(qs, ids)], dtype=np.float32),
                      np.full(n, -1, dtype=np.int64), THRESHOLDS[0], directory)
    s.PREDICTION_PROBABILITY_THRESHOLD = THRESHOLDS[0]
    a, b, m = out["after_exact"].shape[0], out["after_close"].shape[0], out["after_model"].shape[0]
    assert a == 3 and b - a == 4 and m - b == 5 and (out["final_id"] == -1).sum() == 6, (a, b, m, out["final_id"])
    _save(f"{HERE}/predict_end_to_end.npz",
          truth_titles=_utf8(truth), truth_ids=truth_ids, titles=_utf8(f.title), names=_utf8(f.name),
          candidate_ids=candidate_ids, margins=margins, default_margin=np.float32(MARGIN_DEFAULT), jaccard_gap=gap,
          top_n=np.int64(TOP_N), threshold=np.float64(THRESHOLDS[0]),
          **{name: out[name] for name in ("after_exact", "after_close", "after_model", "saved_index", "saved_id",
                                          "final_id", "final_index")})
    return n, len(truth), float(gap.min())


# ---- predict_two_chunks.npz: generate_test_predictions itself over two chunks -------------------------------------------

def _two_chunks(predict, c, s, directory):
    """The reference's generate_test_predictions (predict.py:274-321) on the 10,003 titles of tests/chunk_cases.py with
    top_n = 2: its own loop cuts them into chunks of 10,000 and 3.  MatchMaker in the predict module is the stand-in."""
    import time
    import pandas as pd
    started = time.perf_counter()
    cc = chunk_cases
    truth, truth_ids, titles = cc.truth_titles(), cc.truth_ids(), cc.titles()
    candidate_ids, planted = truth_ids[cc.rows()], cc.probabilities()
    n = len(titles)
    own_top_n, own_class = s.TOP_N_RESULTS_TO_FIND_FOR_PREDICTING, predict.MatchMaker
    s.TOP_N_RESULTS_TO_FIND_FOR_PREDICTING = cc.TOP_N
    s.PREDICTION_PROBABILITY_THRESHOLD = THRESHOLDS[0]
    s.FINAL_OUTPUT_FILE = f"{directory}/final_output_two_chunks.csv"
    predict.MatchMaker = lambda data, truth_data, top_n: _MatchMaker(candidate_ids)
    p = predict.Prediction.__new__(predict.Prediction)
    p.fe = types.SimpleNamespace(
        data=pd.DataFrame({c.COLUMN_TEST_INDEX: np.arange(n), c.COLUMN_TRANSFORMED_TITLE: titles}),
        truth_data=pd.DataFrame({c.COLUMN_TITLE_ID: truth_ids, c.COLUMN_TRANSFORMED_TITLE: truth}),
        space_code=np.uint8(1), number_of_truth_titles=np.uint32(len(truth)))
    p.test_indexes = list(range(n))
    p.model = _PlantedModel()
    p.predictions_columns = [c.COLUMN_TEST_INDEX, c.COLUMN_TRANSFORMED_TITLE, c.COLUMN_MATCH_TRANSFORMED_TITLE,
                             c.COLUMN_MATCH_TITLE_ID, c.COLUMN_PREDICTION]
    p.predictions = pd.DataFrame(index=[], columns=p.predictions_columns)
    p.mapping_title_encoding = {i: np.zeros(255, dtype=np.uint8) for i in range(n)}
    p.mapping_truth_title_encoding = {int(i): np.zeros(255, dtype=np.uint8) for i in truth_ids}
    p.mapping_truth_words_counts = {int(i): np.zeros(15, dtype=np.uint32) for i in truth_ids}
    chunks = []

    def with_planted(remaining, single_prediction=False):       # the stand-in model answers for the rows of `remaining`
        q = np.asarray(remaining[c.COLUMN_TEST_INDEX], dtype=np.int64)
        chunks.append(np.unique(q))
        p.model.planted = planted[q, np.arange(q.shape[0]) % cc.TOP_N]
        return predict.Prediction._find_matches_using_model(p, remaining, single_prediction=single_prediction)

    p._find_matches_using_model = with_planted
    try:
        assert p.generate_test_predictions() == s.FINAL_OUTPUT_FILE
    finally:
        s.TOP_N_RESULTS_TO_FIND_FOR_PREDICTING, predict.MatchMaker = own_top_n, own_class
    final = pd.read_csv(s.FINAL_OUTPUT_FILE, sep=s.TEST_FILE_DELIMITER)
    final_id = np.asarray(final[c.COLUMN_TITLE_ID], dtype=np.int64)
    assert np.array_equal(np.asarray(final[c.COLUMN_TEST_INDEX]), np.arange(n))
    assert len(chunks) == 2 and chunks[0].max() < cc.CHUNK <= chunks[1].min()
    assert np.array_equal(final_id[cc.CHUNK:], final_id[1:4])                  # a title's answer does not depend on its chunk
    saved = p.predictions
    _save(f"{HERE}/predict_two_chunks.npz", final_id=final_id,
          saved_index=np.asarray(saved[c.COLUMN_TEST_INDEX], dtype=np.int64),
          saved_id=np.asarray(saved[c.COLUMN_MATCH_TITLE_ID], dtype=np.int64),
          saved_prediction=np.asarray(saved[c.COLUMN_PREDICTION], dtype=np.float32),
          second_chunk_model_titles=chunks[1])
    return n, int((final_id == -1).sum()), time.perf_counter() - started


def main():
    directory = tempfile.mkdtemp(prefix="ds_golden_predict_")
    os.environ["PROJECT_DATA_PATH"] = directory
    _install_stand_ins()
    sys.path.insert(0, REFERENCE)
    warnings.simplefilter("ignore")

    import doppelspeller.constants as c
    import doppelspeller.settings as s
    from doppelspeller import cli, common, match_maker, predict, train

    assert common.ratio is ratio
    predict.construct_features = lambda *args: None
    try:
        objective = _objective(train, s)
        stages = _stages(predict, common, cli, c, s, directory)
        end_to_end = _end_to_end(predict, common, match_maker, cli, c, s, directory)
        two_chunks = _two_chunks(predict, c, s, directory)
    finally:
        shutil.rmtree(directory)
    print(f"train_objective.npz: {objective[0]} rows, {objective[1]} where the typings differ after quantisation; "
          f"{objective[2]} planted probabilities, typings disagree on {objective[3]} rows per threshold")
    print(f"predict_stages.npz: {stages[0]} title pairs; {stages[1]} titles against {stages[2]} truth rows; "
          f"counts per threshold {stages[3]}")
    print(f"predict_end_to_end.npz: {end_to_end[0]} titles against {end_to_end[1]} truth rows behind the reference's "
          f"MatchMaker, smallest Jaccard gap at the cut of the top {TOP_N}: {end_to_end[2]:.3f}")
    print(f"predict_two_chunks.npz: {two_chunks[0]} titles in two chunks, {two_chunks[1]} not found, "
          f"{two_chunks[2]:.1f} s")


if __name__ == "__main__":
    main()
