"""NumPy restatement of the metric rule ("Metrics"), written from the rule and not from the kernels:
the AUC integers of a score vector by sorting and searching integer keys, and the fixed-point weighted log loss."""
import numpy as np

LOGLOSS_QUANTUM = 1 << 20
LOGLOSS_CAP = 2048.0
NAN_KEY = np.uint32(0xFFFFFFFF)


def keys(scores):
    """uint32 keys of float32 scores whose order is the scores': NaN -> 0xFFFFFFFF, -0.0 as +0.0, else all bits flipped
    for a set sign bit and only the sign bit flipped otherwise."""
    scores = np.ascontiguousarray(scores, dtype=np.float32)
    bits = scores.view(np.uint32).copy()
    nan = (bits & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    bits[bits == np.uint32(0x80000000)] = 0
    negative = (bits & np.uint32(0x80000000)) != 0
    out = np.where(negative, ~bits, bits ^ np.uint32(0x80000000)).astype(np.uint32)
    out[nan] = NAN_KEY
    return out


def auc_counts(scores, labels):
    """(concordant, ties, positives, negatives, nan_rows) as Python ints: np.sort of the negatives' keys, searchsorted
    left / right of the positives' keys.  A row with a NaN score belongs to neither class."""
    key = keys(scores)
    labels = np.asarray(labels)
    valid = key != NAN_KEY
    negatives = np.sort(key[valid & (labels == 0)])
    positives = key[valid & (labels != 0)]
    below = np.searchsorted(negatives, positives, side="left").astype(np.int64)
    not_above = np.searchsorted(negatives, positives, side="right").astype(np.int64)
    return (int(below.sum()), int((not_above - below).sum()), int(positives.shape[0]), int(negatives.shape[0]),
            int(np.count_nonzero(~valid)))


def auc_counts_brute(scores, labels):
    """The same five integers by comparing every (positive, negative) pair: O(|P| |N|)."""
    key = keys(scores).astype(np.int64)
    labels = np.asarray(labels)
    valid = key != int(NAN_KEY)
    positives, negatives = key[valid & (labels != 0)], key[valid & (labels == 0)]
    concordant = ties = 0
    for p in positives:
        concordant += int(np.count_nonzero(negatives < p))
        ties += int(np.count_nonzero(negatives == p))
    return concordant, ties, int(positives.shape[0]), int(negatives.shape[0]), int(np.count_nonzero(~valid))


def auc(counts):
    pairs = counts[2] * counts[3]
    return (2 * counts[0] + counts[1]) / (2 * pairs) if pairs else float("nan")


def softplus(x):
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def logloss_terms(margins, labels, beta):
    """uint64 per row: y * softplus(-m) + beta * (1 - y) * softplus(m) in float64 from the float32 margin, saturated at
    2^11 (a NaN term too), as rint(term * 2^20).  With y in {0, 1} one product vanishes and only the other is taken:
    the same bits for a finite margin, and 0 instead of 0 * inf = NaN for an infinite margin on the row's own side."""
    m = np.ascontiguousarray(margins, dtype=np.float32).astype(np.float64)
    positive = np.asarray(labels) != 0
    with np.errstate(invalid="ignore", over="ignore"):
        term = np.where(positive, softplus(-m), float(beta) * softplus(m))
    term = np.fmin(term, LOGLOSS_CAP)
    return np.rint(term * LOGLOSS_QUANTUM).astype(np.uint64)


def logloss_counts(margins, labels, beta):
    """(fixed-point sum, rows)"""
    terms = logloss_terms(margins, labels, beta)
    return int(terms.sum(dtype=np.uint64)), int(terms.shape[0])


def logloss(counts):
    return counts[0] / LOGLOSS_QUANTUM / counts[1] if counts[1] else float("nan")
