"""The alignment rule and the profile generator of "Edit scripts and the learned misspelling model" (DESIGN.md section 8,
include/doppel_amd.h) restated in plain Python / NumPy from the rule's text, not from csrc/ds_edits.hip: the yardstick of
ds_edit_align, ds_misspell_titles_profile and doppel-speller_amd/edits.py.

Titles are lists of codes (space 1, a-z 2..27, 0-9 28..37).  `a` is the correct title, `b` the observed one."""
import numpy as np

import training_set_oracle as ts

MATCH, SUBSTITUTE, DELETE, INSERT, TRANSPOSE = range(5)
OPS_STRIDE = 512
CODES = 38
MAX_EDITS_LIMIT = 32
# the counts block, int64 offsets
COUNTED, SKIPPED, EDITS = 0, 1, 2
SEEN = EDITS + 33
MATCHED = SEEN + CODES
DELETED = MATCHED + CODES
SUBSTITUTED = DELETED + CODES
INSERTED = SUBSTITUTED + CODES * CODES
TRANSPOSED = INSERTED + CODES * CODES
COUNTS = TRANSPOSED + CODES * CODES
PURPOSE_PROFILE = 8
SCALE = 1 << 30
MAX_COUNT = 1 << 40


def distance_table(a, b):
    """D[i][j], the optimal-string-alignment distance of a[:i] and b[:j]."""
    m, n = len(a), len(b)
    D = [[0] * (n + 1) for _ in range(m + 1)]
    for i in range(m + 1):
        D[i][0] = i
    for j in range(n + 1):
        D[0][j] = j
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            best = min(D[i - 1][j - 1] + (a[i - 1] != b[j - 1]), D[i - 1][j] + 1, D[i][j - 1] + 1)
            if i > 1 and j > 1 and a[i - 1] == b[j - 2] and a[i - 2] == b[j - 1]:
                best = min(best, D[i - 2][j - 2] + 1)
            D[i][j] = best
    return D


def align(a, b):
    """(distance, script): the script is the reversed traceback, one operation per entry."""
    D = distance_table(a, b)
    i, j = len(a), len(b)
    script = []
    while i > 0 or j > 0:
        if i > 0 and j > 0 and a[i - 1] == b[j - 1] and D[i][j] == D[i - 1][j - 1]:
            script.append(MATCH)
            i, j = i - 1, j - 1
        elif i > 0 and j > 0 and D[i][j] == D[i - 1][j - 1] + 1:
            script.append(SUBSTITUTE)
            i, j = i - 1, j - 1
        elif i > 1 and j > 1 and a[i - 1] == b[j - 2] and a[i - 2] == b[j - 1] and D[i][j] == D[i - 2][j - 2] + 1:
            script.append(TRANSPOSE)
            i, j = i - 2, j - 2
        elif i > 0 and D[i][j] == D[i - 1][j] + 1:
            script.append(DELETE)
            i -= 1
        else:
            script.append(INSERT)
            j -= 1
    return D[len(a)][len(b)], script[::-1]


def walk(a, b, script):
    """(operation, i, j) per entry of a script, i and j the characters of a and b consumed before it."""
    i = j = 0
    for op in script:
        yield op, i, j
        i += {MATCH: 1, SUBSTITUTE: 1, DELETE: 1, INSERT: 0, TRANSPOSE: 2}[op]
        j += {MATCH: 1, SUBSTITUTE: 1, DELETE: 0, INSERT: 1, TRANSPOSE: 2}[op]


def new_counts():
    return np.zeros(COUNTS, dtype=np.int64)


def count_pair(counts, a, b, distance, script, max_edits):
    """Adds one pair to the block."""
    if distance > max_edits:
        counts[SKIPPED] += 1
        return
    counts[COUNTED] += 1
    counts[EDITS + distance] += 1
    counts[SEEN] += 1
    for code in a:
        counts[SEEN + code] += 1
    for op, i, j in walk(a, b, script):
        if op == MATCH:
            counts[MATCHED + a[i]] += 1
        elif op == SUBSTITUTE:
            counts[SUBSTITUTED + a[i] * CODES + b[j]] += 1
        elif op == DELETE:
            counts[DELETED + a[i]] += 1
        elif op == INSERT:
            context = a[i] if i < len(a) else 0
            counts[INSERTED + context * CODES + b[j]] += 1
        else:
            counts[TRANSPOSED + a[i] * CODES + a[i + 1]] += 1


def align_batch(truth, truth_rows, observed, observed_rows, max_edits, counts=None):
    """ds_edit_align of the pairs (truth[truth_rows[p]], observed[observed_rows[p]]); truth / observed are lists of code
    lists, a row array may be None.  Returns (distance int32[n], ops uint8[n, 512] zero-filled, lengths int32[n], counts);
    `counts` is added to when given."""
    assert 0 <= max_edits <= MAX_EDITS_LIMIT
    n = len(truth) if truth_rows is None else len(truth_rows)
    counts = new_counts() if counts is None else counts
    distance = np.zeros(n, np.int32)
    ops = np.zeros((n, OPS_STRIDE), np.uint8)
    lengths = np.zeros(n, np.int32)
    cache = {}
    for p in range(n):
        ra = p if truth_rows is None else int(truth_rows[p])
        rb = p if observed_rows is None else int(observed_rows[p])
        a, b = truth[ra], observed[rb]
        if (ra, rb) not in cache:
            cache[ra, rb] = align(a, b)
        d, script = cache[ra, rb]
        distance[p], lengths[p] = d, len(script)
        ops[p, :len(script)] = script
        count_pair(counts, a, b, d, script, max_edits)
    return distance, ops, lengths, counts


class Views:
    """The named views of a counts block."""

    def __init__(self, counts):
        counts = np.asarray(counts, dtype=np.int64)
        assert counts.shape == (COUNTS,)
        self.counts = counts
        self.edits = counts[EDITS:EDITS + 33]
        self.seen = counts[SEEN:SEEN + CODES]
        self.match = counts[MATCHED:MATCHED + CODES]
        self.delete = counts[DELETED:DELETED + CODES]
        self.substitute = counts[SUBSTITUTED:SUBSTITUTED + CODES * CODES].reshape(CODES, CODES)
        self.insert = counts[INSERTED:INSERTED + CODES * CODES].reshape(CODES, CODES)
        self.transpose = counts[TRANSPOSED:TRANSPOSED + CODES * CODES].reshape(CODES, CODES)


class Profile(Views):
    """A counts block the generator accepts (a ValueError otherwise) and the integer rates it derives from it."""

    def __init__(self, counts):
        Views.__init__(self, counts)
        problem = self.problem()
        if problem:
            raise ValueError(problem)

        def rate(events, c):
            return 0 if self.seen[c] == 0 else (SCALE * int(events)) // int(self.seen[c])
        self.rate_sub = [rate(self.substitute[c].sum() - self.substitute[c, c], c) for c in range(CODES)]
        self.rate_del = [rate(self.delete[c], c) for c in range(CODES)]
        self.rate_tr = [rate(self.transpose[c].sum(), c) for c in range(CODES)]
        self.rate_ins = [rate(self.insert[c].sum(), c) for c in range(CODES)]
        if max(self.rate_sub + self.rate_del + self.rate_tr + self.rate_ins) >= 1 << 32:
            raise ValueError("a rate is 4 events per seen character or more")

    def problem(self):
        c = self.counts
        if (c < 0).any() or (c >= MAX_COUNT).any():
            return "a count is negative or not below 2^40"
        if self.edits[1:].sum() == 0:
            return "edits[1..32] are all 0"
        if self.match[0] or self.delete[0] or self.substitute[0].any() or self.substitute[:, 0].any() or \
                np.diagonal(self.substitute).any() or self.insert[:, 0].any() or self.transpose[0].any() or \
                self.transpose[:, 0].any():
            return "a count that no alignment produces is not 0"
        return None


def _draw_code(rng, row, skip):
    weights = [0 if y == skip else int(row[y]) for y in range(CODES)]
    r = rng.below(sum(weights))
    for y, weight in enumerate(weights):
        if r < weight:
            return y
        r -= weight
    raise AssertionError("the row is empty")


def _weights(profile, w, p):
    L = len(w)
    if p < L:
        c = w[p]
        sub = profile.rate_sub[c]
        delete = 0 if L <= 3 else profile.rate_del[c]
        tr = profile.rate_tr[c] if p + 1 < L and w[p] != w[p + 1] else 0
    else:
        c, sub, delete, tr = 0, 0, 0, 0
    ins = 0 if L >= ts.MAX_CHARACTERS else profile.rate_ins[c]
    return sub, delete, tr, ins


def misspell_profile_codes(codes, seed, row, profile):
    """ds_misspell_titles_profile of one title: the stream of (seed, 8, row)."""
    rng = ts.Stream(seed, PURPOSE_PROFILE, row)
    drawn = rng.below(int(profile.edits[1:].sum()))
    k, cumulative = 0, 0
    while True:
        k += 1
        cumulative += int(profile.edits[k])
        if cumulative > drawn:
            break
    w = list(codes)
    for _ in range(k):
        total = sum(sum(_weights(profile, w, p)) for p in range(len(w) + 1))
        if total == 0:
            break
        r = rng.below(total)
        done = False
        for p in range(len(w) + 1):
            for operation, weight in enumerate(_weights(profile, w, p)):
                if r >= weight:
                    r -= weight
                    continue
                if operation == 0:
                    w[p] = _draw_code(rng, profile.substitute[w[p]], w[p])
                elif operation == 1:
                    del w[p]
                elif operation == 2:
                    w[p], w[p + 1] = w[p + 1], w[p]
                else:
                    w.insert(p, _draw_code(rng, profile.insert[w[p] if p < len(w) else 0], -1))
                done = True
                break
            if done:
                break
    return ts.transform_codes(w)


def misspell_profile(title, seed, row, profile):
    return ts.to_text(misspell_profile_codes(ts.to_codes(title), seed, row, profile))
