"""The rule of the exhaustive stage (include/doppel_amd.h, DESIGN.md section 8 "Exhaustive matches") restated twice, and the
crafted probabilities the tests fold.

    best_rows          NumPy, whole arrays at once: what the kernels and Prediction.exhaustive_matches are compared against
    best_rows_python   a query at a time with sorted(): what best_rows is compared against

Per query, over truth rows row_first .. row_first + N - 1 with one probability each: the n rows with the largest float32
BITS of the probability, the lower row first among equal bits; an unfilled slot (N < n) is (-1, quiet NaN 0x7fc00000)."""
import numpy as np

EMPTY_PROBABILITY = np.array([0x7fc00000], dtype=np.uint32).view(np.float32)[0]


def best_rows(probabilities, n, row_first=0):
    """probabilities float32[Q, N] -> (row int32[Q, n], probability float32[Q, n])"""
    probabilities = np.ascontiguousarray(probabilities, dtype=np.float32)
    n_queries, n_rows = probabilities.shape
    bits = probabilities.view(np.uint32).astype(np.uint64)
    row = np.broadcast_to(np.arange(n_rows, dtype=np.uint64) + np.uint64(row_first), probabilities.shape)
    # descending (bits, -row) = ascending (~bits, row)
    order = np.argsort(((np.uint64(0xffffffff) - bits) << np.uint64(32)) | row, axis=1, kind="stable")[:, :n]
    out_row = np.full((n_queries, n), -1, dtype=np.int32)
    out_probability = np.full((n_queries, n), EMPTY_PROBABILITY, dtype=np.float32)
    filled = min(n, n_rows)
    out_row[:, :filled] = order + row_first
    out_probability[:, :filled] = np.take_along_axis(probabilities, order, axis=1)
    return out_row, out_probability


def best_rows_python(probabilities, n, row_first=0):
    """The same lists, one query at a time: [[(row, probability bits)] * n] * Q."""
    bits = np.ascontiguousarray(probabilities, dtype=np.float32).view(np.uint32)
    out = []
    for q in range(bits.shape[0]):
        ranked = sorted(range(bits.shape[1]), key=lambda t: (-int(bits[q, t]), t))[:n]
        out.append([(row_first + t, int(bits[q, t])) for t in ranked] + [(-1, 0x7fc00000)] * (n - len(ranked)))
    return out


def best_keys(probabilities, n, row_first=0):
    """uint64[Q, n]: the running list the fold leaves, (bits << 32) | (0xffffffff - row) descending, 0 = empty."""
    return keys_of(best_rows(probabilities, n, row_first))


def keys_of(best):
    """best_keys from the lists best_rows has already returned (a long table is sorted once)."""
    row, probability = best
    bits = np.ascontiguousarray(probability).view(np.uint32).astype(np.uint64)
    keys = (bits << np.uint64(32)) | (np.uint64(0xffffffff) - np.maximum(row, 0).astype(np.uint64))
    return np.where(row >= 0, keys, np.uint64(0))


def as_lists(best):
    """best_rows' arrays in the form of best_rows_python."""
    row, probability = best
    bits = np.ascontiguousarray(probability).view(np.uint32)
    return [[(int(row[q, s]), int(bits[q, s])) for s in range(row.shape[1])] for q in range(row.shape[0])]


def same_best(a, b):
    """Bit for bit: the probabilities compared as their uint32 bits (the empty slots hold a NaN)."""
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
               and x.dtype == y.dtype and x.shape == y.shape for x, y in zip(a, b))


KINDS = ("random", "equal", "few", "zeros", "straddle")


def make_probabilities(n_queries, n_rows, kind, seed=0, marks=()):
    """float32[Q, N], finite and non-negative:
         random    distinct values in no order         few     four values: ties everywhere
         equal     one value: the lowest rows win      zeros   +0.0 but for a few rows
         straddle  the one maximum at every row of `marks` and at both ends (rows either side of a slice boundary or a
                   call boundary), a lower value elsewhere: the ties must come out in row order across the boundaries"""
    rng = np.random.RandomState(seed)
    if kind == "random":
        values = rng.permutation(n_queries * n_rows).reshape(n_queries, n_rows) / np.float32(n_queries * n_rows)
    elif kind == "equal":
        values = np.full((n_queries, n_rows), 0.625)
    elif kind == "few":
        values = rng.randint(0, 4, size=(n_queries, n_rows)) / 4.0
    elif kind == "zeros":
        values = np.zeros((n_queries, n_rows))
        values[:, rng.randint(0, n_rows, max(1, n_rows // 7))] = 0.5
    else:
        values = rng.randint(0, 3, size=(n_queries, n_rows)) / 8.0
        for mark in (0, n_rows - 1) + tuple(marks):
            if 0 <= mark < n_rows:
                values[:, mark] = 0.875
    return np.ascontiguousarray(values, dtype=np.float32)


def planted_units(rows):
    """The order in which make_planted's values fall over the sorted `rows`, before the shuffle: pairs of equal values
    (the lower row first; the partner lies half the list further on, as far away as the rows allow) and single rows."""
    rows = sorted(int(r) for r in rows)
    half = len(rows) // 2
    paired = set(range(0, half, 2))
    return [(rows[i], rows[i + half]) for i in sorted(paired)] + \
           [(rows[i],) for i in range(len(rows)) if i not in paired and i - half not in paired]


def make_planted(n_rows, n, seed, rows=None):
    """float32[1, n_rows] whose n best rows are known without a sort, and those rows int32[1, n] in the order of the rule.
    The backdrop is the "few" kind halved (0, 1/8, 1/4, 3/8: ties everywhere, none can win).  On top, n values >= 0.5 at
    `rows` (n distinct rows of the caller's; default: spread evenly, rows 0 and n_rows - 1 among them).  The units of
    planted_units(rows) are shuffled and take descending values 0.5 + k / 256, so both rows of a pair hold the SAME bits
    and the lower row must come first, however far apart the two are."""
    rng = np.random.RandomState(seed)
    values = make_probabilities(1, n_rows, "few", seed=seed) * np.float32(0.5)
    if rows is None:
        rows = [0] if n == 1 else [s * (n_rows - 1) // (n - 1) for s in range(n)]
    assert len(set(rows)) == len(rows) == n <= min(n_rows, 64) and 0 <= min(rows) and max(rows) < n_rows
    units = planted_units(rows)
    units = [units[u] for u in rng.permutation(len(units))]
    winners = []
    for position, unit in enumerate(units):
        values[0, list(unit)] = np.float32(0.5 + (len(units) - position) / 256.0)
        winners += unit
    return values, np.array([winners], dtype=np.int32)


def fold_levels(n_rows, n, slice_keys=4096):
    """Slices per query at every level of the fold of one tile of n_rows rows: level 0 holds the rows and the running list
    of n keys, every further level the n keys of each slice of the level before, until one slice is left."""
    slices, keys = [], n_rows + n
    while not slices or slices[-1] > 1:
        slices.append(-(-keys // slice_keys))
        keys = slices[-1] * n
    return slices


def split(n_rows, calls):
    """The [first, last) row ranges of `calls` folds of one table with a ragged last call (fewer where N is small)."""
    size = -(-n_rows // calls) + (1 if calls > 1 and n_rows % calls == 0 and n_rows > calls else 0)
    return [(first, min(n_rows, first + size)) for first in range(0, n_rows, max(1, size))]
