"""NumPy restatement of the model-inspection rule ("Model inspection"; csrc/ds_inspect.hip).

A job (kind, feature, value, repeat) changes one value of every row before the forest is walked:
    BASELINE  nothing
    PERMUTE   row[feature] = rows[perm(i)][feature]
    OVERRIDE  row[feature] = value
The margin of the changed row is float32(base_margin) + the float32 sum of the leaves from zero in tree order (the rule
of csrc/ds_forest.h).  Per job five integers: tp, tn, fp, fn (predicted positive iff sigmoid(margin) > threshold,
actual positive iff target != 0, a null target is all 0) and margin_sum = the sum of
rint(clip(float64(margin), -2^11, 2^11) * 2^20), a NaN margin adding 0 and counting as not positive.

The probability here is the float64 sigmoid of the exact float32 margin; the device takes a float32 expf.  The cases
keep every probability away from the threshold (probability_gap), so the counts are the same.
"""
import numpy as np

MASK = (1 << 64) - 1
BASELINE, PERMUTE, OVERRIDE = 0, 1, 2
PURPOSE_PERMUTE = 6
QUANTUM = 1 << 20
CAP = 2048.0


# ---- the permutation ---------------------------------------------------------------------------------------------------
def sample_key(seed, purpose, index):
    """The first kept (third) output of the splitmix64 stream of (seed, purpose, index): csrc/ds_train.h."""
    z = (seed * 0x9e3779b97f4a7c15 + index * 0xd1342543de82ef95 + purpose * 0xaf251af3b0f025b5 +
         3 * 0x9e3779b97f4a7c15) & MASK
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & MASK
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & MASK
    return z ^ (z >> 31)


def mix64(x):
    x ^= x >> 30
    x = (x * 0xbf58476d1ce4e5b9) & MASK
    x ^= x >> 27
    x = (x * 0x94d049bb133111eb) & MASK
    return x ^ (x >> 31)


def round_keys(seed, feature, repeat):
    return [sample_key(seed, PURPOSE_PERMUTE, (repeat << 40) | (feature << 32) | j) for j in range(4)]


def half_bits(n):
    return max(1, ((n - 1).bit_length() + 1) // 2)


def perm_one(seed, feature, repeat, n, i):
    """perm(i), in plain Python integers."""
    if n == 1:
        return 0
    b = half_bits(n)
    mask = (1 << b) - 1
    keys = round_keys(seed, feature, repeat)
    x = i
    while True:
        left, right = x >> b, x & mask
        for key in keys:
            left, right = right, left ^ (mix64(key ^ right) & mask)
        x = (left << b) | right
        if x < n:
            return x


def _mix64_array(x):
    x = x ^ (x >> np.uint64(30))
    x = x * np.uint64(0xbf58476d1ce4e5b9)
    x = x ^ (x >> np.uint64(27))
    x = x * np.uint64(0x94d049bb133111eb)
    return x ^ (x >> np.uint64(31))


def perm(seed, feature, repeat, n):
    """int64[n]: perm(i) for every i (the same rule on uint64 arrays, which wrap like the device's integers)."""
    if n == 1:
        return np.zeros(1, np.int64)
    b = np.uint64(half_bits(n))
    mask = np.uint64((1 << int(b)) - 1)
    keys = [np.uint64(key) for key in round_keys(seed, feature, repeat)]
    x = np.arange(n, dtype=np.uint64)
    walking = np.arange(n)
    while walking.shape[0]:
        left, right = x[walking] >> b, x[walking] & mask
        for key in keys:
            left, right = right, left ^ (_mix64_array(key ^ right) & mask)
        x[walking] = (left << b) | right
        walking = walking[x[walking] >= np.uint64(n)]
    return x.astype(np.int64)


# ---- the forest ----------------------------------------------------------------------------------------------------------
def leaf_sums(forest, rows):
    """float32[n]: the leaves of every row summed from zero in tree order in float32, all rows of a tree at a time."""
    feature, threshold = forest["feature"], forest["threshold"]
    n = rows.shape[0]
    total = np.zeros(n, np.float32)
    for t in range(forest["tree_offsets"].shape[0] - 1):
        root = int(forest["tree_offsets"][t])
        node = np.full(n, root, np.int64)
        while True:
            inner = np.flatnonzero(feature[node] >= 0)
            if inner.shape[0] == 0:
                break
            at = node[inner]
            value = rows[inner, feature[at]]
            with np.errstate(invalid="ignore"):
                below = value < threshold[at]
            step = np.where(np.isnan(value), forest["missing"][at], np.where(below, forest["yes"][at], forest["no"][at]))
            node[inner] = root + step
        total = (total + threshold[node]).astype(np.float32)
    return total


def margins(forest, rows):
    return (np.float32(forest["base_margin"]) + leaf_sums(forest, rows)).astype(np.float32)


def changed_rows(rows, job, seed):
    kind, feature, value, repeat = job
    if kind == BASELINE:
        return rows
    out = rows.copy()
    if kind == PERMUTE:
        out[:, feature] = rows[perm(seed, feature, repeat, rows.shape[0]), feature]
    else:
        assert kind == OVERRIDE
        out[:, feature] = np.float32(value)
    return out


def job_key(job):
    kind, feature, value, repeat = job
    if kind == BASELINE:
        return (BASELINE,)
    if kind == PERMUTE:
        return (PERMUTE, int(feature), int(repeat))
    return (OVERRIDE, int(feature), np.float32(value).tobytes())


def probabilities(margin):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-margin.astype(np.float64)))


def counters_of(margin, target, threshold):
    """The five integers of one job from its float32 margins."""
    positive = probabilities(margin) > threshold          # False for a NaN
    actual = np.zeros(margin.shape[0], bool) if target is None else np.asarray(target) != 0
    wide = margin.astype(np.float64)
    terms = np.where(np.isnan(wide), 0.0, np.rint(np.clip(wide, -CAP, CAP) * QUANTUM)).astype(np.int64)
    return [int(np.count_nonzero(positive & actual)), int(np.count_nonzero(~positive & ~actual)),
            int(np.count_nonzero(positive & ~actual)), int(np.count_nonzero(~positive & actual)), int(terms.sum())]


def inspect(forest, rows, target, jobs, seed, threshold=0.9):
    """(uint64[n_jobs, 5] with margin_sum in two's complement, the smallest |probability - threshold| over all rows and
    jobs).  Jobs that change the rows in the same way are walked once."""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    seen = {}
    out = np.zeros((len(jobs), 5), dtype=np.int64)
    gap = np.inf
    for at, job in enumerate(jobs):
        key = job_key(job)
        if key not in seen:
            margin = margins(forest, changed_rows(rows, job, seed))
            distance = np.abs(probabilities(margin) - threshold)
            seen[key] = (counters_of(margin, target, threshold), float(np.nanmin(distance)) if rows.shape[0] else np.inf)
        out[at] = seen[key][0]
        gap = min(gap, seen[key][1])
    return out.view(np.uint64), gap


# ---- what the host derives from the integers ---------------------------------------------------------------------------------
def permutation_jobs(features, n_repeats):
    return [(BASELINE, 0, 0.0, 0)] + [(PERMUTE, int(f), 0.0, r) for f in features for r in range(n_repeats)]


def dependence_jobs(feature, grid):
    return [(BASELINE, 0, 0.0, 0)] + [(OVERRIDE, int(feature), np.float32(v), 0) for v in grid]


def permutation_importance(counters, n, n_selected, n_repeats, beta=5.0):
    """dict of the derived arrays of PermutationImportance, float64 from the integers."""
    counts = counters.view(np.int64)
    baseline = tuple(int(v) for v in counts[0, :4])
    baseline_error = baseline[3] + beta * baseline[2]
    matrix = counts[1:, :4].reshape(n_selected, n_repeats, 4)
    errors = matrix[:, :, 3].astype(np.float64) + beta * matrix[:, :, 2].astype(np.float64)
    shift = (counts[1:, 4] - counts[0, 4]).astype(np.float64).reshape(n_selected, n_repeats) / QUANTUM / n
    return dict(baseline=baseline, baseline_error=baseline_error, error_matrix=matrix, errors=errors,
                importance=(errors - baseline_error).mean(axis=1), importance_std=(errors - baseline_error).std(axis=1),
                margin_shift=shift.mean(axis=1))


def importance_order(features, importance):
    """Positions by importance, descending, ties to the lower feature."""
    return sorted(range(len(features)), key=lambda s: (-importance[s], features[s]))


def quantile_grid(column, n_grid):
    """The default grid of partial_dependence: the distinct values among n_grid evenly spaced order statistics of the
    column's non-NaN values, ascending, and one NaN last when the column has any."""
    column = np.asarray(column, dtype=np.float32)
    values = sorted(float(v) for v in column if not np.isnan(v))
    picked = sorted({values[(k * (len(values) - 1)) // max(n_grid - 1, 1)] for k in range(n_grid)}) if values else []
    if np.isnan(column).any():
        picked.append(float("nan"))
    return np.array(picked, dtype=np.float32)


def partial_dependence(counters, n):
    counts = counters.view(np.int64)
    return dict(baseline_mean_margin=float(counts[0, 4]) / QUANTUM / n,
                mean_margin=counts[1:, 4].astype(np.float64) / QUANTUM / n,
                positive_share=(counts[1:, 0] + counts[1:, 2]).astype(np.float64) / n)
