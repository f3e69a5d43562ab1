"""Hostile float32 values for every place that maps a raw value to a tree branch ("Order of
values"), shared by test_value_cases_cpu.py and test_gpu_value_edges.py: the crafted columns of cuts_cases.py with
evaluation rows on, one step below and one step above every cut, a forest whose thresholds are such values, a matrix
that fills the whole cut table, and an independent reference that orders values by the integer key of csrc/ds_radix.h's
header comment, restated here in NumPy.  Everything is generated from seeds; nothing here calls the code under test.

The rule: IEEE comparison with denormals kept, -0.0 == +0.0, a NaN value follows `missing`, nothing is below a NaN
threshold, and x < cut iff bin(x) < b for cut = cuts[b - 1]."""
import functools

import numpy as np

import cuts_cases
import forest_continue_oracle as continued
import forest_train_oracle as oracle

FLT_MAX = np.finfo(np.float32).max
TINY = np.float32(1e-45)                      # the smallest denormal, bits 0x00000001
ALWAYS = np.array([np.inf, -np.inf, 0.0, -0.0, TINY, -TINY, FLT_MAX, -FLT_MAX], np.float32)
REPLICAS = 3                                  # the extra values of a column, shuffled against the other columns anew
NAN_ROWS = 24                                 # every column keeps at least this many NaNs per replica
TRAINED = dict(rounds=12, max_depth=4, eta=0.3, min_child_weight=1.0, reg_lambda=1.0)


# ---- the integer order -------------------------------------------------------------------------------------------------
def key(values):
    """uint32 keys of float32 values: 0xFFFFFFFF for a NaN, else with -0.0 read as +0.0 the bits with all bits flipped
    when the sign is set and only the sign bit flipped otherwise.  Ascending keys are ascending values."""
    bits = np.ascontiguousarray(values, dtype=np.float32).view(np.uint32).copy()
    nan = (bits & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)
    bits[bits == np.uint32(0x80000000)] = np.uint32(0)
    negative = (bits & np.uint32(0x80000000)) != 0
    out = np.where(negative, ~bits, bits ^ np.uint32(0x80000000)).astype(np.uint32)
    out[nan] = np.uint32(0xffffffff)
    return out


def is_nan(values):
    return key(values) == np.uint32(0xffffffff)


def below(values, thresholds):
    """bool: value < threshold by keys alone; False for a NaN on either side."""
    kv, kt = key(values), key(thresholds)
    return (kv < kt) & (kv != np.uint32(0xffffffff)) & (kt != np.uint32(0xffffffff))


def key_bins(rows, per_feature):
    """uint8[n_features, n]: per value the number of the feature's cuts whose key is <= the value's, 255 for a NaN."""
    rows = np.asarray(rows, dtype=np.float32)
    out = np.empty((rows.shape[1], rows.shape[0]), np.uint8)
    for f, feature_cuts in enumerate(per_feature):
        values = key(rows[:, f])
        count = (key(feature_cuts)[None, :] <= values[:, None]).sum(axis=1)
        out[f] = np.where(values == np.uint32(0xffffffff), oracle.MISSING, count)
    return out


def key_walk(arrays, rows):
    """(int64[n_trees, n]: the node, in the model's node order, of the leaf every row reaches in every tree;
    int64[n_nodes]: the rows that visit each node).  A NaN value follows `missing`; any other follows `yes` when its
    key is below the threshold's and the threshold is no NaN, else `no`."""
    rows = np.asarray(rows, dtype=np.float32)
    n, offsets = rows.shape[0], np.asarray(arrays["tree_offsets"])
    leaves = np.zeros((offsets.shape[0] - 1, n), np.int64)
    counts = np.zeros(arrays["feature"].shape[0], np.int64)
    everyone = np.arange(n)
    for t in range(offsets.shape[0] - 1):
        root = int(offsets[t])
        node = np.full(n, root, np.int64)
        moving = everyone
        while moving.shape[0]:
            counts += np.bincount(node[moving], minlength=counts.shape[0])
            moving = moving[arrays["feature"][node[moving]] >= 0]
            at = node[moving]
            value = rows[moving, arrays["feature"][at]]
            step = np.where(is_nan(value), arrays["missing"][at],
                            np.where(below(value, arrays["threshold"][at]), arrays["yes"][at], arrays["no"][at]))
            node[moving] = root + step
        leaves[t] = node
    return leaves, counts


def leaf_sums(arrays, leaves):
    """float32[n]: the leaf values of key_walk's leaves summed from zero in tree order in float32."""
    total = np.zeros(leaves.shape[1], np.float32)
    for t in range(leaves.shape[0]):
        total = (total + arrays["threshold"][leaves[t]]).astype(np.float32)
    return total


# ---- the hostile matrix ------------------------------------------------------------------------------------------------
class Hostile:
    """rows float32[n, 22]: the crafted part first (n_train rows, the training rows), then the extra rows (evaluation
    and prediction rows only); names: the columns; cuts: forest_train_oracle.cuts of the crafted part at max_bin."""

    def __init__(self, rows, names, n_train, cuts, max_bin):
        self.rows, self.names, self.n_train, self.cuts, self.max_bin = rows, names, n_train, cuts, max_bin
        self.train, self.extra = rows[:n_train], rows[n_train:]
        self.y, self.extra_y = labels(self.train, names), labels(self.extra, names)


def neighbours(values):
    """Every value, the float32 just below it and the float32 just above it."""
    values = np.asarray(values, dtype=np.float32)
    with np.errstate(over="ignore"):                                    # the step beyond +-FLT_MAX is +-inf
        return np.concatenate([values, np.nextafter(values, np.float32(-np.inf)),
                               np.nextafter(values, np.float32(np.inf))])


def labels(rows, names):
    """y = (score >= 3) of six terms of the crafted columns (a NaN satisfies none)."""
    column = lambda name: rows[:, names.index(name)]
    with np.errstate(invalid="ignore"):
        score = (column("denormals") > 0).astype(np.int64) + (column("infinities") == np.inf) + \
            (column("signed_zeros") >= 0) + (column("shared_low_mixed") > 0) + (column("denormals_few") > 0) + \
            (np.nan_to_num(column("nan_30")) > 0.3)
    return (score >= 3).astype(np.float32)


@functools.lru_cache(maxsize=None)
def hostile_matrix(max_bin=256):
    """cuts_cases.crafted_matrix() with extra rows: for every feature each of its cuts, the float32 below and above it,
    +-inf, +-0.0, +-1e-45 and +-FLT_MAX, NaN for the rest; REPLICAS times, every column shuffled on its own each time so
    that a value meets other neighbours.  The arrays are shared: read only."""
    crafted, names = cuts_cases.crafted_matrix()
    per_feature = oracle.cuts(crafted, max_bin)
    values = [np.concatenate([neighbours(c), ALWAYS]) for c in per_feature]
    height = max(v.shape[0] for v in values) + NAN_ROWS
    rng = np.random.RandomState(1000 + max_bin)
    blocks = []
    for _ in range(REPLICAS):
        block = np.full((height, crafted.shape[1]), np.nan, np.float32)
        for f, v in enumerate(values):
            block[:v.shape[0], f] = v
            rng.shuffle(block[:, f])
        blocks.append(block)
    rows = np.ascontiguousarray(np.concatenate([crafted] + blocks), dtype=np.float32)
    rows.setflags(write=False)
    return Hostile(rows, names, crafted.shape[0], per_feature, max_bin)


@functools.lru_cache(maxsize=None)
def oracle_trained(max_bin=256):
    """The flat arrays of the twelve depth-4 trees the oracle grows on the crafted part (TRAINED), NumPy's sigmoid."""
    h = hostile_matrix(max_bin)
    q = TRAINED
    trees, _ = oracle.train(h.train, h.y, q["rounds"], q["max_depth"], q["eta"], q["min_child_weight"], q["reg_lambda"],
                            max_bin=max_bin)
    return continued.flat_forest([continued.flat_tree(tree, h.cuts) for tree in trees])


def threshold_census(arrays):
    """(denormal, equal to 0.0, equal to +inf): the split thresholds of a forest of each kind."""
    t = arrays["threshold"][arrays["feature"] >= 0]
    bits = t.view(np.uint32)
    denormal = ((bits & np.uint32(0x7f800000)) == 0) & ((bits & np.uint32(0x007fffff)) != 0)
    return int(denormal.sum()), int((t == 0).sum()), int((t == np.inf).sum())


# ---- a forest of hostile thresholds ------------------------------------------------------------------------------------
def _tree(nodes):
    """One tree from a list of nodes: a float (a leaf) or (feature, threshold, yes, no, missing)."""
    size = len(nodes)
    out = dict(feature=np.full(size, -1, np.int32), threshold=np.zeros(size, np.float32), yes=np.zeros(size, np.int32),
               no=np.zeros(size, np.int32), missing=np.zeros(size, np.int32))
    for i, node in enumerate(nodes):
        if isinstance(node, tuple):
            out["feature"][i], out["threshold"][i], out["yes"][i], out["no"][i], out["missing"][i] = node
        else:
            out["threshold"][i] = node
    return out


def _written_trees(names):
    """The paths the issue names.  In each a NaN of the repeated feature travels along the repeated splits, so that
    every split can be left through `missing` too.
    A: `< +inf`, then `>= -inf`, then a third split, all on `infinities`.
    B: `denormals` three times, narrowing to the negative denormals, then to the smallest one.
    C: `signed_zeros` at +0.0 (which -0.0 is not below), at the smallest denormal (which both zeros are below) and at 1.
    D: a NaN threshold and a -inf threshold, whose `yes` children no value reaches, then -0.0, which +0.0 is not below."""
    inf, den, zero, few = (names.index(n) for n in ("infinities", "denormals", "signed_zeros", "denormals_few"))
    a = _tree([(inf, np.inf, 1, 2, 1), (inf, -np.inf, 3, 4, 4), 0.5, -0.125, (inf, 0.0, 5, 6, 5), 0.25, -0.375])
    b = _tree([(den, 0.0, 1, 2, 1), (den, np.float32(-5e-39), 3, 4, 4), (few, TINY, 5, 6, 5), 0.3125,
               (den, -TINY, 7, 8, 7), 0.1875, -0.0625, -0.4375, 0.09375])
    c = _tree([(zero, 0.0, 1, 2, 2), -0.21875, (zero, TINY, 3, 4, 4), 0.40625, (zero, 1.0, 5, 6, 5), 0.15625, -0.28125])
    d = _tree([(few, np.nan, 1, 2, 1), 0.71875, (inf, -np.inf, 3, 4, 4), -0.65625, (zero, -0.0, 5, 6, 6),
               0.53125, -0.59375])
    return [a, b, c, d]


def _pool(column, feature_cuts, rng):
    """Thresholds for one feature: values of the column and of its cuts with their float32 neighbours, the constants
    every column gets, and NaN."""
    present = column[~np.isnan(column)]
    own = rng.choice(present, min(12, present.shape[0]), replace=False) if present.shape[0] else np.zeros(0, np.float32)
    some_cuts = rng.choice(feature_cuts, min(12, feature_cuts.shape[0]), replace=False) if feature_cuts.shape[0] \
        else np.zeros(0, np.float32)
    return np.concatenate([neighbours(own), neighbours(some_cuts), ALWAYS, ALWAYS,
                           np.array([np.nan], np.float32)]).astype(np.float32)


def _grown_tree(rng, rows, pools, depth):
    """A random tree in breadth-first order whose every split sends at least one of `rows` to each of `yes`, `no` and
    `missing`, where the threshold lets a value go `yes` at all (a NaN or -inf threshold does not).  A third of the
    splits below the root take a feature already on their path, so that bounds merge."""
    nodes, frontier = [None], [(0, 0, np.arange(rows.shape[0]), [])]
    while frontier:
        at, level, reach, path = frontier.pop(0)
        split = None
        if level < depth and reach.shape[0] and not (level >= 2 and rng.rand() < 0.15):
            for _ in range(60):
                f = int(rng.choice(path)) if path and rng.rand() < 0.35 else int(rng.randint(rows.shape[1]))
                cut = np.float32(rng.choice(pools[f]))
                value = rows[reach, f]
                nan = is_nan(value)
                yes = below(value, np.full(value.shape, cut, np.float32))
                no = ~nan & ~yes
                barren = bool(is_nan(np.float32(cut))) or cut == -np.inf
                if nan.any() and no.any() and (yes.any() or barren):
                    split = (f, cut, nan, yes, no)
                    break
        if split is None:
            nodes[at] = float(np.float32(rng.randint(-16, 17) / 32.0 + rng.randint(1, 8) / 256.0))
            continue
        f, cut, nan, yes, no = split
        to_yes = rng.rand() < 0.5
        left, right = len(nodes), len(nodes) + 1
        nodes += [None, None]
        nodes[at] = (f, cut, left, right, left if to_yes else right)
        frontier.append((left, level + 1, reach[yes | (nan & to_yes)], path + [f]))
        frontier.append((right, level + 1, reach[no | (nan & (not to_yes))], path + [f]))
    return _tree(nodes)


@functools.lru_cache(maxsize=None)
def hostile_forest(seed=0):
    """Flat arrays (base margin 0) of proper binary trees of depth <= 6 over the 22 columns: the written trees above and
    nine grown ones (13 trees: the inspection kernel walks trees two at a time and the odd one on its own) whose
    thresholds are drawn from the columns' own values and cuts, their float32 neighbours, +-0.0, +-inf, +-FLT_MAX, the
    smallest denormals and NaN; `missing` to either side.  The rows that guide the grown trees are those of
    hostile_matrix(256).  Leaves are multiples of 2^-8 in (-0.6, 0.6)."""
    h = hostile_matrix(256)
    rng = np.random.RandomState(seed)
    pools = [_pool(h.train[:, f], h.cuts[f], rng) for f in range(h.rows.shape[1])]
    trees = _written_trees(h.names) + [_grown_tree(rng, h.rows, pools, 6 if t % 2 else 5) for t in range(9)]
    forest = continued.flat_forest(trees)
    for array in forest.values():
        if isinstance(array, np.ndarray):
            array.setflags(write=False)
    return forest


def tree_depths(arrays):
    """The number of splits on the longest root-to-leaf path of every tree."""
    out = []
    for t in range(arrays["tree_offsets"].shape[0] - 1):
        begin, end = int(arrays["tree_offsets"][t]), int(arrays["tree_offsets"][t + 1])
        depth = np.zeros(end - begin, np.int64)
        for i in range(end - begin):                                    # children come after their parent
            if arrays["feature"][begin + i] >= 0:
                depth[arrays["yes"][begin + i]] = depth[arrays["no"][begin + i]] = depth[i] + 1
        out.append(int(depth.max()))
    return out


def paths(arrays):
    """Every root-to-leaf path as a list of (node, went_yes), node in the model's node order."""
    out = []
    for t in range(arrays["tree_offsets"].shape[0] - 1):
        begin = int(arrays["tree_offsets"][t])
        stack = [(begin, [])]
        while stack:
            node, path = stack.pop()
            if arrays["feature"][node] < 0:
                out.append(path)
                continue
            stack.append((begin + int(arrays["yes"][node]), path + [(node, True)]))
            stack.append((begin + int(arrays["no"][node]), path + [(node, False)]))
    return out


def _scalar_key(value):
    return int(key(np.float32(value))[0])


def merged_bounds(arrays):
    """[(feature, lo, hi, splits)] for every feature of every root-to-leaf path: lo the largest threshold the path
    leaves through `no` (value >= lo), hi the smallest it leaves through `yes` (value < hi), by key; None without such a
    split; NaN thresholds bound nothing.  splits: how many of the path's splits are on the feature."""
    out = []
    for path in paths(arrays):
        per_feature = {}
        for node, went_yes in path:
            per_feature.setdefault(int(arrays["feature"][node]), []).append((arrays["threshold"][node], went_yes))
        for f, splits in per_feature.items():
            lo = [t for t, went_yes in splits if not went_yes and not is_nan(np.float32(t))]
            hi = [t for t, went_yes in splits if went_yes and not is_nan(np.float32(t))]
            out.append((f, max(lo, key=_scalar_key) if lo else None,
                        min(hi, key=_scalar_key) if hi else None, len(splits)))
    return out


def inspection_grid(arrays, feature):
    """partial_dependence's explicit grid for one feature: every threshold of its splits, the float32 below and above
    each, +-0.0, +-inf and NaN, in a fixed order without repeated bit patterns."""
    cuts = arrays["threshold"][arrays["feature"] == feature]
    cuts = cuts[~is_nan(cuts)]
    grid = np.concatenate([neighbours(cuts), np.array([0.0, -0.0, np.inf, -np.inf, np.nan], np.float32)])
    _, first = np.unique(grid.view(np.uint32), return_index=True)
    return np.ascontiguousarray(grid[np.sort(first)], dtype=np.float32)


# ---- a matrix that fills the cut table ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def full_table_matrix(n=1000):
    """float32[n, 96], every column with at least 255 distinct values, so that each gets 254 cuts at max_bin 256 and the
    bin kernel reads all 96 * 254 entries of its cut table.  Columns 0, 3, 6, .. hold denormals of both signs; column
    1 has exactly 255 distinct values; columns 4 and 7 hold two -inf and five +inf (so that +inf is their last cut),
    columns 5 and 8 a fifth of NaNs, column 10 both.  Read only."""
    assert n >= 600
    rng = np.random.RandomState(96)
    x = np.empty((n, 96), np.float32)
    for f in range(96):
        if f % 3 == 0:
            draws = rng.randint(1, 1 << 23, 2 * n).astype(np.uint32)
            bits = draws[np.sort(np.unique(draws, return_index=True)[1])][:n]
            assert bits.shape[0] == n
            bits[rng.rand(n) < 0.5] |= np.uint32(0x80000000)
            x[:, f] = bits.view(np.float32)
        elif f == 1:
            x[:, f] = (np.arange(n) % 255).astype(np.float32) * np.float32(0.25) - np.float32(31.0)
            rng.shuffle(x[:, f])
        else:
            x[:, f] = (rng.permutation(n).astype(np.float32) - np.float32(n // 2)) * np.float32(2.0 ** (f % 7 - 3))
        if f in (4, 7, 10):
            order = np.argsort(x[:, f])
            x[order[:2], f] = -np.inf
            x[order[-5:], f] = np.inf
        if f in (5, 8, 10):
            x[rng.rand(n) < 0.2, f] = np.nan
    x.setflags(write=False)
    return x
