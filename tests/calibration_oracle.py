"""The calibration rule ("Calibration") restated in NumPy and Python integers: the key order, the
isotonic fit by stack pooling on exact integers, its level sets, the step map, raw_threshold and the reliability
integers.  No device code: what the kernels of ds_calibrate.hip are compared with."""
from fractions import Fraction

import numpy as np

NAN_KEY = 0xFFFFFFFF
FLT_MAX = np.float32(np.finfo(np.float32).max)
SCALE = float(1 << 30)


def cut_key(values):
    """uint32 keys of float32 values (ds_radix.h): ascending keys = ascending values, -0.0 as +0.0, a NaN 0xFFFFFFFF."""
    bits = np.ascontiguousarray(values, dtype=np.float32).view(np.uint32).astype(np.uint64)
    bits = np.where(bits == 0x80000000, 0, bits)
    keys = np.where(bits & 0x80000000, ~bits & 0xFFFFFFFF, bits ^ 0x80000000)
    return np.where((bits & 0x7FFFFFFF) > 0x7F800000, NAN_KEY, keys).astype(np.uint32)


def key_value(keys):
    """float32 values of keys (none of them the NaN key)."""
    keys = np.asarray(keys, dtype=np.uint64)
    bits = np.where(keys & 0x80000000, keys ^ 0x80000000, ~keys & 0xFFFFFFFF)
    return bits.astype(np.uint32).view(np.float32)


def points(scores, target):
    """(keys uint32[D] ascending and distinct, pos int[D], neg int[D], n_nan)."""
    keys = cut_key(scores)
    positive = np.asarray(target, dtype=np.float32) != 0
    kept = keys != NAN_KEY
    distinct, inverse = np.unique(keys[kept], return_inverse=True)
    pos = np.bincount(inverse, weights=positive[kept], minlength=distinct.shape[0]).astype(np.int64)
    total = np.bincount(inverse, minlength=distinct.shape[0]).astype(np.int64)
    return distinct, pos, total - pos, int((~kept).sum())


def pool(pos, neg):
    """Stack pooling of the points on Python integers -> [first point, pos, neg] per level set.  A block joins the one
    before it when that one's mean is not below its own."""
    stack = []
    for at, (p, q) in enumerate(zip(pos.tolist(), neg.tolist())):
        block = [at, p, q]
        while stack and stack[-1][1] * (block[1] + block[2]) >= block[1] * (stack[-1][1] + stack[-1][2]):
            first, p0, q0 = stack.pop()
            block = [first, p0 + block[1], q0 + block[2]]
        stack.append(block)
    return stack


def fit(scores, target):
    """The level sets: dict(lo float32[K], hi float32[K], pos int64[K], neg int64[K], n_nan, n_points)."""
    keys, pos, neg, n_nan = points(scores, target)
    blocks = pool(pos, neg)
    first = np.array([b[0] for b in blocks], dtype=np.int64)
    last = np.append(first[1:], keys.shape[0])[:first.shape[0]] - 1
    return dict(lo=key_value(keys[first]), hi=key_value(keys[last]),
                pos=np.array([b[1] for b in blocks], dtype=np.int64),
                neg=np.array([b[2] for b in blocks], dtype=np.int64), n_nan=n_nan, n_points=int(keys.shape[0]))


def brute_force(pos, neg):
    """fit_i = max over a <= i of min over b >= i of mean(a .. b), in Fractions, per point."""
    count = len(pos)
    cp, ct = [0], [0]
    for p, q in zip(pos, neg):
        cp.append(cp[-1] + int(p))
        ct.append(ct[-1] + int(p) + int(q))
    # least[a][i] = min over b >= i of mean(a .. b), as a running minimum from the right: count^2 fractions in all
    least = []
    for a in range(count):
        row, running = [None] * count, None
        for b in range(count - 1, a - 1, -1):
            mean = Fraction(cp[b + 1] - cp[a], ct[b + 1] - ct[a])
            running = mean if running is None or mean < running else running
            row[b] = running
        least.append(row)
    return [max(least[a][i] for a in range(i + 1)) for i in range(count)]


def values(pos, neg):
    """float64 pos / (pos + neg) per block."""
    pos, neg = np.asarray(pos, dtype=np.int64), np.asarray(neg, dtype=np.int64)
    return pos.astype(np.float64) / (pos + neg).astype(np.float64)


def transform(lo, value, scores):
    """The step map in float32: value of the last block whose lo is not above the score; 0 below lo[0]; NaN for a NaN
    score or without blocks."""
    scores = np.ascontiguousarray(scores, dtype=np.float32)
    out = np.full(scores.shape, np.nan, dtype=np.float32)
    keys = cut_key(scores)
    value = np.asarray(value, dtype=np.float64).astype(np.float32)
    if value.shape[0] == 0:
        return out
    at = np.searchsorted(cut_key(lo), keys, side="right")
    mapped = np.where(at > 0, value[np.maximum(at, 1) - 1], np.float32(0))
    return np.where(keys == NAN_KEY, np.float32(np.nan), mapped).astype(np.float32)


def raw_threshold(lo, value, q):
    """float32 t with (score > t) exactly where transform(score) > q: just below the first block whose float32 value
    exceeds q; -FLT_MAX when that is block 0, +FLT_MAX when there is none."""
    above = np.nonzero(np.asarray(value, dtype=np.float64).astype(np.float32).astype(np.float64) > float(q))[0]
    if above.shape[0] == 0:
        return FLT_MAX
    if above[0] == 0:
        return -FLT_MAX
    return np.nextafter(np.float32(lo[above[0]]), np.float32(-np.inf))


def neighbours(edges):
    """Every edge, the float32 just below and just above it, and a NaN."""
    edges = np.ascontiguousarray(edges, dtype=np.float32)
    return np.concatenate([edges, np.nextafter(edges, np.float32(-np.inf)), np.nextafter(edges, np.float32(np.inf)),
                           np.array([np.nan], dtype=np.float32)])


def reliability(probabilities, target, n_bins):
    """int64[n_bins + 1][4]: rows, positives, sum rint(p * 2^30), sum rint((p - y)^2 * 2^30) per bin; the last row
    takes the probabilities that are NaN or outside [0, 1] (rows and positives only)."""
    p = np.ascontiguousarray(probabilities, dtype=np.float32).astype(np.float64)
    y = (np.asarray(target, dtype=np.float32) != 0)
    out = np.zeros((n_bins + 1, 4), dtype=np.int64)
    with np.errstate(invalid="ignore"):
        inside = (p >= 0.0) & (p <= 1.0)
    out[n_bins, 0] = int((~inside).sum())
    out[n_bins, 1] = int((~inside & y).sum())
    p, y = p[inside], y[inside]
    bins = np.minimum(np.floor(p * n_bins).astype(np.int64), n_bins - 1)
    miss = p - y.astype(np.float64)
    for column, addend in enumerate((np.ones_like(bins), y.astype(np.int64), np.rint(p * SCALE).astype(np.int64),
                                     np.rint(miss * miss * SCALE).astype(np.int64))):
        np.add.at(out[:, column], bins, addend)
    return out
