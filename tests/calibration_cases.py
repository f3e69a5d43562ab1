"""Named small inputs of the calibration kernels, built from nothing but the code below.  The sizes sit on the edges of
the kernels (wave 64, workgroup 256, the sort's tile of 8192 keys, the head scan's tile of 2048 elements, the default
segment of 1024 points), not on those of the workload."""
import numpy as np

FLT_MAX = np.finfo(np.float32).max
DENORMAL = np.float32(1e-45)


def _f32(values):
    return np.ascontiguousarray(values, dtype=np.float32)


def _alternating(n):
    return _f32(np.arange(n)), _f32(np.arange(n) % 2 == 0)          # 1 0 1 0 ...: every pair violates


def _staircase(negatives=150000):
    # The 3043 reduced fractions p / q with q <= 100 in ascending order, point i holding p positives of q rows: the rates
    # rise strictly, so no segment pools anything at the first level.  Then two points of 150000 negatives each with the
    # highest scores: the last level pools them back across every segment boundary.
    from math import gcd
    steps = sorted(((p, q) for q in range(2, 101) for p in range(1, q) if gcd(p, q) == 1), key=lambda f: f[0] / f[1])
    # With negatives = 0 the 3043 points are the answer: more blocks than the last level's stack keeps in LDS (2048).
    scores = np.concatenate([np.full(q, i, np.float32) for i, (p, q) in enumerate(steps)] +
                            [np.full(negatives, 5000, np.float32), np.full(negatives, 5001, np.float32)])
    target = np.concatenate([_f32([1] * p + [0] * (q - p)) for p, q in steps] + [np.zeros(2 * negatives, np.float32)])
    return scores, target


def _equal_means():
    # points (1 of 2), (2 of 4), (1 of 2), (3 of 6): one block of value 1/2; then (1 of 3) drags them all to 8/17, and
    # (0 of 1) before them stays apart
    rows = [(0.0, 0, 1), (1.0, 1, 1), (2.0, 2, 2), (3.0, 1, 1), (4.0, 3, 3), (5.0, 1, 2), (6.0, 1, 0), (7.0, 1, 0)]
    scores, target = [], []
    for score, pos, neg in rows:
        scores += [score] * (pos + neg)
        target += [1.0] * pos + [0.0] * neg
    return _f32(scores), _f32(target)


def _random(seed, n, distinct, nan_share=0.0):
    rng = np.random.default_rng(seed)
    scores = _f32(rng.integers(0, distinct, n)) / np.float32(distinct)
    target = _f32(rng.random(n) < scores * 0.8 + 0.1)
    if nan_share:
        scores[rng.random(n) < nan_share] = np.nan
    return scores, target


def fit_cases():
    """name -> (scores float32[n], target float32[n])."""
    cases = {
        "empty": (_f32([]), _f32([])),
        "one_positive": (_f32([0.5]), _f32([1])),
        "one_negative": (_f32([0.5]), _f32([0])),
        "two_ordered": (_f32([0.25, 0.75]), _f32([0, 1])),
        "two_reversed": (_f32([0.25, 0.75]), _f32([1, 0])),
        "positives_only": (_f32([0.1, 0.2, 0.3, 0.2]), _f32([1, 1, 2, 1])),
        "negatives_only": (_f32([0.1, 0.2, 0.3, 0.2]), _f32([0, 0, 0, 0])),
        "all_equal_mixed": (_f32([0.5] * 7), _f32([1, 0, 0, 1, 1, 0, 1])),
        "separated": (_f32([0.1, 0.2, 0.3, 0.7, 0.8, 0.9]), _f32([0, 0, 0, 1, 1, 1])),
        "reversed": (_f32(np.arange(100)), _f32(np.arange(100) < 50)),
        "staircase_then_negatives": _staircase(),
        "staircase": _staircase(0),
        "equal_means": _equal_means(),
        "zeros": (_f32([0.0, -0.0, -0.0, 0.0, 1.0, -1.0]), _f32([1, 0, 1, 0, 1, 0])),
        "extremes": (_f32([-np.inf, -FLT_MAX, -1.0, -DENORMAL, 0.0, DENORMAL, 1.0, FLT_MAX, np.inf, np.inf, -np.inf]),
                     _f32([0, 1, 0, 0, 1, 0, 1, 1, 1, 0, 1])),
        "nan_scattered": (_f32([np.nan, 0.1, 0.9, np.nan, 0.5, -np.nan, 0.5, 0.2]), _f32([1, 0, 1, 0, 1, 1, 0, 1])),
        "nan_only": (_f32([np.nan, np.nan, -np.nan]), _f32([1, 0, 1])),
        "saturated": (_f32([0.0] * 5 + [1.0] * 5 + [0.5] * 4), _f32([0, 0, 1, 0, 0, 1, 1, 1, 0, 1, 1, 0, 1, 0])),
        "random_300": _random(1, 300, 40),
        "random_5000_nan": _random(2, 5000, 3000, nan_share=0.01),
        "random_20000": _random(3, 20000, 1 << 20),
    }
    for n in (63, 64, 65, 257, 8191, 8192, 8193, 3 * 8192 + 5):
        cases[f"alternating_{n}"] = _alternating(n)
    return cases


def reliability_cases():
    """name -> (probabilities float32[n], target float32[n], n_bins)."""
    edges = _f32(np.arange(11) / 10.0)
    wide = _f32([0.0, -0.0, 1.0, 0.5, np.nextafter(np.float32(1), np.float32(0)), -0.25, 1.5, np.nan, np.inf, -np.inf,
                 DENORMAL, 0.3])
    rng = np.random.default_rng(7)
    many = _f32(rng.random(3000))
    return {
        "bin_edges_10": (np.concatenate([edges, edges]), _f32([1] * 11 + [0] * 11), 10),
        "outside_and_ends_10": (wide, _f32(np.arange(wide.shape[0]) % 2), 10),
        "one_bin": (wide, _f32(np.arange(wide.shape[0]) % 3 == 0), 1),
        "bins_256": (np.concatenate([many, _f32(np.arange(257) / 256.0)]),
                     _f32(np.concatenate([rng.random(3000) < many, np.arange(257) % 2])), 256),
        "empty": (_f32([]), _f32([]), 10),
    }
