"""The cases of the model-inspection tests (test_inspect_cpu.py, test_gpu_inspect.py): forests from random_dump and
matrices from random_rows (test_forest_cpu.py), with job tables and targets, at the smallest shapes where the kernel of
csrc/ds_inspect.hip can still go wrong: one row, one short wave, a whole wave and one more, a whole workgroup and one
more, three row blocks; 1, 3, 7, 66 and 96 features; no tree, stumps, depth 6 and one tree of depth 16; 0, 1, 2 and 3
trees, at which the kernel's two-trees-at-a-time walk takes no pair, only the tree left over, one pair exactly, and one
pair and a tree left over.

Every case must keep all of its probabilities (every row under every job) at least PROBABILITY_GAP away from the
threshold, so that the float32 expf of the device (within 2 ulp of libm by the project's own bound; 1e-6 is about four
float32 ulps of 0.9) cannot count a row differently from the float64 sigmoid of the oracle.  test_inspect_cpu.py
asserts it; a seed that fails is replaced here, not tolerated."""
import functools

import numpy as np

import forest_inspect_oracle as oracle
from forest_inspect_oracle import BASELINE, OVERRIDE, PERMUTE
from test_forest_cpu import random_dump, random_rows

PROBABILITY_GAP = 1e-6
THRESHOLD = 0.9


def forest_of(seed, n_trees, n_features, depth, base_score=0.5):
    from doppel_speller_amd.forest import ForestModel
    return ForestModel.parse_xgboost_dump(random_dump(seed, n_trees=n_trees, n_features=n_features, depth=depth),
                                          base_score=base_score)


def every_feature(n_features, repeats=3):
    return oracle.permutation_jobs(range(n_features), repeats)


def override_jobs(forest, feature):
    """NaN, both infinities, the threshold of a split on `feature` and the float32 just below it."""
    cuts = forest["threshold"][forest["feature"] == feature]
    assert cuts.shape[0], "the forest must split on the feature"
    cut = np.float32(cuts[0])
    values = [np.nan, np.inf, -np.inf, cut, np.nextafter(cut, np.float32(-np.inf), dtype=np.float32)]
    return [(OVERRIDE, feature, np.float32(v), 0) for v in values]


def target_of(kind, n, seed):
    if kind == "null":
        return None
    if kind == "zeros":
        return np.zeros(n, np.float32)
    if kind == "ones":
        return np.ones(n, np.float32)
    assert kind == "mixed"
    return (np.random.RandomState(seed).rand(n) < 0.4).astype(np.float32)


#      name                 n  features  forest (seed, trees, depth)  target   matrix seed
SHAPES = [
    ("one_row",             1,  1, (11, 5, 1), "ones", 21),
    ("two_rows",            2,  7, (12, 12, 6), "mixed", 22),
    ("no_trees",           63, 66, (13, 0, 6), "zeros", 23),
    ("single_baseline",    64, 66, (14, 40, 6), "null", 24),
    ("wide_matrix",        65, 96, (15, 10, 6), "mixed", 25),
    ("deep_tree",         255,  7, (16, 1, 16), "mixed", 26),
    ("one_workgroup",     256, 66, (17, 40, 6), "mixed", 27),
    ("stumps",            257, 66, (18, 20, 1), "ones", 28),
    ("three_row_blocks",  700, 66, (19, 40, 6), "mixed", 39),
    ("base_margin",       700,  7, (20, 30, 6), "null", 30),
    ("many_job_groups",     2,  1, (31, 3, 1), "mixed", 32),
    ("two_trees",          65,  3, (33, 2, 2), "mixed", 34),
]


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(name, forest, n_features, rows, target, jobs, seed, expected (uint64[n_jobs, 5]), gap)."""
    name_, n, n_features, (forest_seed, n_trees, depth), target_kind, rows_seed = next(s for s in SHAPES if s[0] == name)
    base_score = 0.25 if name == "base_margin" else 0.5
    forest = forest_of(forest_seed, n_trees, n_features, depth, base_score)
    rows = random_rows(rows_seed, n, n_features)
    if name == "three_row_blocks":                                   # the one matrix without NaNs
        rows = np.random.RandomState(rows_seed).uniform(0, 100, (n, n_features)).astype(np.float32)
    if name == "single_baseline":
        jobs = [(BASELINE, 0, 0.0, 0)]
    elif name == "no_trees":
        jobs = oracle.permutation_jobs([0, 65], 2) + [(OVERRIDE, 3, np.float32(np.nan), 0)]
    elif name == "deep_tree":
        feature = int(forest["feature"][0])
        jobs = every_feature(n_features) + override_jobs(forest, feature)
    elif name == "base_margin":
        feature = int(forest["feature"][0])
        jobs = every_feature(n_features, 2) + override_jobs(forest, feature) + [(BASELINE, 5, 1.0, 9)]
    elif name == "many_job_groups":                                  # more job groups than the grid's second dimension holds
        values = [np.nan, 0.0, 50.0, 99.0, np.inf]
        jobs = [(BASELINE, 0, 0.0, 0)] + [(OVERRIDE, 0, np.float32(values[j % 5]), 0) if j % 3 else (PERMUTE, 0, 0.0, j % 4)
                                          for j in range(70000)]
    else:
        jobs = every_feature(n_features)
    seed = forest_seed * 1000003 + 7
    target = target_of(target_kind, n, rows_seed)
    expected, gap = oracle.inspect(forest, rows, target, jobs, seed, THRESHOLD)
    return dict(name=name, forest=forest, n_features=n_features, rows=rows, target=target, jobs=jobs, seed=seed,
                expected=expected, gap=gap)


NAMES = [shape[0] for shape in SHAPES]
