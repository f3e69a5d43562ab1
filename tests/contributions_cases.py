"""Yardsticks of the contributions stage (include/doppel_amd.h, DESIGN.md section 8 "Contributions") in plain NumPy float64:

    tree_shap            Lundberg, Erion and Lee 2018, Algorithm 2 as published (RECURSE / EXTEND / UNWIND), recursive over
                         the nodes; every quantity is a vector over the rows, which changes no row's arithmetic
    shapley_brute_force  the Shapley definition over all subsets of the features a tree uses, the value of a subset being
                         Algorithm 1's path-dependent expectation (EXPVALUE)
    saabas               the change of the subtree mean along the row's own path
    node_counts          the cover, by walking rows on the host

and forests that force the awkward cases.  A forest is the `arrays` dict of ForestModel (feature, threshold, yes, no,
missing, tree_offsets, base_margin); a cover is float64[n_nodes] in the same node order."""
import itertools
import math

import numpy as np

from test_forest_cpu import random_dump, random_rows  # noqa: F401  (re-exported for the tests)

TOL_FACTOR = 1e-10          # the device tolerance per entry is TOL_FACTOR * forest_scale(forest)


def base_margin(forest):
    """The base margin as the model holds it: a float32."""
    return float(np.float32(forest["base_margin"]))


def forest_scale(forest):
    """S = |base_margin| + the sum over the trees of max |leaf|: what one rounding error of a contribution scales with."""
    total = abs(base_margin(forest))
    offsets = forest["tree_offsets"]
    for t in range(offsets.shape[0] - 1):
        part = slice(int(offsets[t]), int(offsets[t + 1]))
        leaves = forest["feature"][part] < 0
        total += float(np.abs(forest["threshold"][part][leaves].astype(np.float64)).max())
    return total


def leaf_sum_bound(forest):
    """The sum over the trees of max |leaf| (the scale of the forest kernel's float32 margin)."""
    return forest_scale(forest) - abs(base_margin(forest))


def from_trees(trees, base_margin=0.0):
    """A forest from per-tree dicts of feature / threshold / yes / no / missing (tree-relative child ids)."""
    offsets = np.zeros(len(trees) + 1, np.int64)
    offsets[1:] = np.cumsum([len(tree["feature"]) for tree in trees])
    cat = lambda key, dtype: np.concatenate([np.asarray(tree[key]) for tree in trees]).astype(dtype)
    return dict(feature=cat("feature", np.int32), threshold=cat("threshold", np.float32), yes=cat("yes", np.int32),
                no=cat("no", np.int32), missing=cat("missing", np.int32), tree_offsets=offsets,
                base_margin=float(base_margin))


def tree(nodes):
    """One tree from a list of nodes: a float (a leaf) or (feature, threshold, yes, no, missing)."""
    out = dict(feature=[], threshold=[], yes=[], no=[], missing=[])
    for node in nodes:
        split = isinstance(node, tuple)
        out["feature"].append(node[0] if split else -1)
        out["threshold"].append(node[1] if split else node)
        for key, at in (("yes", 2), ("no", 3), ("missing", 4)):
            out[key].append(node[at] if split else 0)
    return out


def chain_tree(depth, n_features, rng):
    """A tree `depth` splits deep: every `yes` child is a leaf, every `no` child the next split (the last one a leaf)."""
    nodes = []
    for level in range(depth):
        at = 2 * level
        nodes.append((level % n_features, float(rng.uniform(10, 90)), at + 1, at + 2, at + 1 + int(rng.rand() < 0.5)))
        nodes.append(float(rng.normal(0, 0.3)))
    nodes.append(float(rng.normal(0, 0.3)))
    return tree(nodes)


def random_tree(rng, features, depth, leaf_chance=0.2, thresholds=(20.0, 35.0, 50.0, 65.0, 80.0)):
    """A random tree in breadth-first order that splits on `features` only, on a few thresholds (so that a feature met
    again on a path narrows, or empties, its interval)."""
    nodes, frontier = [None], [(0, 0)]
    while frontier:
        at, level = frontier.pop(0)
        if level >= depth or (level > 0 and rng.rand() < leaf_chance):
            nodes[at] = float(np.float32(rng.normal(0, 0.3)))
            continue
        yes, no = len(nodes), len(nodes) + 1
        nodes += [None, None]
        nodes[at] = (int(rng.choice(features)), float(rng.choice(thresholds)), yes, no, yes if rng.rand() < 0.5 else no)
        frontier += [(yes, level + 1), (no, level + 1)]
    return tree(nodes)


def small_rows(rng, n, n_features, nan_chance=0.2):
    rows = rng.choice([5.0, 20.0, 30.0, 35.0, 50.0, 60.0, 65.0, 90.0], (n, n_features)).astype(np.float32)
    rows[rng.rand(n, n_features) < nan_chance] = np.nan
    return rows


def additive_cover(forest, leaf_cover):
    """A cover whose leaves hold leaf_cover (per node; read at the leaves only) and whose inner nodes are the sum of
    their children."""
    cover = np.asarray(leaf_cover, dtype=np.float64).copy()
    offsets = forest["tree_offsets"]
    for t in range(offsets.shape[0] - 1):
        begin, end = int(offsets[t]), int(offsets[t + 1])
        for i in range(end - 1, begin - 1, -1):
            if forest["feature"][i] >= 0:
                cover[i] = cover[begin + forest["yes"][i]] + cover[begin + forest["no"][i]]
    return cover


def _goes_yes(forest, node, rows):
    """bool[n]: the rows that leave `node` (global id) through its `yes` child, by the rule of ds_forest_kernel."""
    value = rows[:, forest["feature"][node]]
    missing_yes = forest["missing"][node] == forest["yes"][node]
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(value), missing_yes, value < forest["threshold"][node])


def _children(forest, at, rows, which):
    """The tree-relative child each of rows[which] takes at its node at[i] (global ids), by the rule of ds_forest_kernel."""
    value = rows[which, forest["feature"][at]]
    with np.errstate(invalid="ignore"):
        below = value < forest["threshold"][at]
    return np.where(np.isnan(value), forest["missing"][at], np.where(below, forest["yes"][at], forest["no"][at]))


def node_counts(forest, rows):
    """int64[n_nodes]: the rows that visit each node."""
    rows = np.asarray(rows, dtype=np.float32)
    counts = np.zeros(forest["feature"].shape[0], dtype=np.int64)
    offsets = forest["tree_offsets"]
    for t in range(offsets.shape[0] - 1):
        begin = int(offsets[t])
        node = np.full(rows.shape[0], begin, dtype=np.int64)
        active = np.ones(rows.shape[0], dtype=bool)
        while active.any():
            np.add.at(counts, node[active], 1)
            split = forest["feature"][node] >= 0
            active &= split
            node[active] = begin + _children(forest, node[active], rows, active)
    return counts


def margins64(forest, rows):
    """float64[n]: base_margin plus the leaves the rows reach, summed in float64."""
    rows = np.asarray(rows, dtype=np.float32)
    out = np.full(rows.shape[0], base_margin(forest), dtype=np.float64)
    offsets = forest["tree_offsets"]
    for t in range(offsets.shape[0] - 1):
        begin = int(offsets[t])
        node = np.full(rows.shape[0], begin, dtype=np.int64)
        while (forest["feature"][node] >= 0).any():
            split = forest["feature"][node] >= 0
            node[split] = begin + _children(forest, node[split], rows, split)
        out += forest["threshold"][node].astype(np.float64)
    return out


# ---- Algorithm 2 -----------------------------------------------------------------------------------------------------
class _Path:
    """The unique path m of Algorithm 2: feature d, zero fraction z, one fraction o and weight w per element; z is a
    number, o and w are vectors over the rows."""

    def __init__(self, d=(), z=(), o=(), w=()):
        self.d, self.z, self.o, self.w = list(d), list(z), list(o), list(w)

    def copy(self):
        return _Path(self.d, self.z, self.o, [w.copy() for w in self.w])


def _extend(m, pz, po, pi, n_rows):
    m = m.copy()
    l = len(m.d)
    m.d.append(pi); m.z.append(pz); m.o.append(po)
    m.w.append(np.ones(n_rows) if l == 0 else np.zeros(n_rows))
    for i in range(l - 1, -1, -1):
        m.w[i + 1] = m.w[i + 1] + po * m.w[i] * (i + 1) / (l + 1)
        m.w[i] = pz * m.w[i] * (l - i) / (l + 1)
    return m


def _unwind(m, i):
    l = len(m.d) - 1
    o, z = m.o[i], m.z[i]
    follows = o != 0
    safe = np.where(follows, o, 1.0)
    n = m.w[l]
    out = _Path(m.d[:l], m.z[:l], m.o[:l], [w.copy() for w in m.w[:l]])
    for j in range(l - 1, -1, -1):
        t = out.w[j]
        with_one = n * (l + 1) / ((j + 1) * safe)
        without = out.w[j] * (l + 1) / (z * (l - j))
        out.w[j] = np.where(follows, with_one, without)
        n = np.where(follows, t - with_one * z * (l - j) / (l + 1), n)
    for j in range(i, l):
        out.d[j], out.z[j], out.o[j] = m.d[j + 1], m.z[j + 1], m.o[j + 1]
    return out


def _unwound_sum(m, i):
    return sum(_unwind(m, i).w)


def tree_shap(forest, cover, rows):
    """float64[n, n_features + 1]: Algorithm 2 per tree, summed in tree order; the last column is base_margin plus per
    tree the sum over its leaves of value * the product of cover[child] / cover[parent] down the leaf's path."""
    rows = np.asarray(rows, dtype=np.float32)
    cover = np.asarray(cover, dtype=np.float64)
    n, n_features = rows.shape
    phi = np.zeros((n, n_features + 1), dtype=np.float64)
    phi[:, n_features] = base_margin(forest)
    offsets = forest["tree_offsets"]
    for t in range(offsets.shape[0] - 1):
        begin = int(offsets[t])
        expectation = [0.0]

        def recurse(j, m, pz, po, pi, reach):
            m = _extend(m, pz, po, pi, n)
            if forest["feature"][j] < 0:
                value = float(forest["threshold"][j])
                expectation[0] += value * reach
                for i in range(1, len(m.d)):
                    phi[:, m.d[i]] += _unwound_sum(m, i) * (m.o[i] - m.z[i]) * value
                return
            yes = _goes_yes(forest, j, rows)
            d = int(forest["feature"][j])
            iz, io = 1.0, np.ones(n)
            seen = [k for k in range(1, len(m.d)) if m.d[k] == d]
            if seen:
                iz, io = m.z[seen[0]], m.o[seen[0]]
                m = _unwind(m, seen[0])
            for child, taken in ((begin + int(forest["yes"][j]), yes), (begin + int(forest["no"][j]), ~yes)):
                fraction = cover[child] / cover[j]
                recurse(child, m, iz * fraction, io * taken.astype(np.float64), d, reach * fraction)

        recurse(begin, _Path(), 1.0, np.ones(n), -1, 1.0)
        phi[:, n_features] += expectation[0]
    return phi


# ---- the Shapley definition over Algorithm 1's expectation ---------------------------------------------------------------
def _expected_value(forest, cover, rows, begin, node, subset):
    """EXPVALUE of Algorithm 1 for every row: follow the row at a split on a feature of `subset`, else weigh both
    children by their share of the node's cover."""
    j = begin + node
    if forest["feature"][j] < 0:
        return np.full(rows.shape[0], float(forest["threshold"][j]))
    yes = _expected_value(forest, cover, rows, begin, int(forest["yes"][j]), subset)
    no = _expected_value(forest, cover, rows, begin, int(forest["no"][j]), subset)
    if int(forest["feature"][j]) in subset:
        return np.where(_goes_yes(forest, j, rows), yes, no)
    return (cover[begin + forest["yes"][j]] * yes + cover[begin + forest["no"][j]] * no) / cover[j]


def shapley_brute_force(forest, cover, rows):
    """float64[n, n_features + 1] by the definition: phi_i = sum over S of |S|! (M - |S| - 1)! / M! * (v(S + i) - v(S))
    over the subsets S of the other features the tree uses; the last column is base_margin + the sum of v(empty)."""
    rows = np.asarray(rows, dtype=np.float32)
    cover = np.asarray(cover, dtype=np.float64)
    n, n_features = rows.shape
    phi = np.zeros((n, n_features + 1), dtype=np.float64)
    phi[:, n_features] = base_margin(forest)
    offsets = forest["tree_offsets"]
    for t in range(offsets.shape[0] - 1):
        begin, end = int(offsets[t]), int(offsets[t + 1])
        used = sorted(set(int(f) for f in forest["feature"][begin:end] if f >= 0))
        assert len(used) <= 8, "too many features to enumerate"
        value = {subset: _expected_value(forest, cover, rows, begin, 0, frozenset(subset))
                 for size in range(len(used) + 1) for subset in itertools.combinations(used, size)}
        phi[:, n_features] += value[()]
        m = len(used)
        for i in used:
            others = [f for f in used if f != i]
            for size in range(m):
                weight = math.factorial(size) * math.factorial(m - size - 1) / math.factorial(m)
                for subset in itertools.combinations(others, size):
                    phi[:, i] += weight * (value[tuple(sorted(subset + (i,)))] - value[subset])
    return phi


# ---- Saabas ----------------------------------------------------------------------------------------------------------
def node_means(forest, cover):
    """float64[n_nodes]: the cover-weighted mean leaf value below every node."""
    mean = np.zeros(forest["feature"].shape[0], dtype=np.float64)
    offsets = forest["tree_offsets"]
    for t in range(offsets.shape[0] - 1):
        begin, end = int(offsets[t]), int(offsets[t + 1])
        for i in range(end - 1, begin - 1, -1):
            if forest["feature"][i] < 0:
                mean[i] = float(forest["threshold"][i])
            else:
                yes, no = begin + forest["yes"][i], begin + forest["no"][i]
                mean[i] = (cover[yes] * mean[yes] + cover[no] * mean[no]) / cover[i]
    return mean


def saabas(forest, cover, rows):
    """float64[n, n_features + 1]: along each row's own path a split adds mean(child) - mean(node) to its feature; the
    last column is base_margin + the sum of the roots' means."""
    rows = np.asarray(rows, dtype=np.float32)
    cover = np.asarray(cover, dtype=np.float64)
    mean = node_means(forest, cover)
    n, n_features = rows.shape
    phi = np.zeros((n, n_features + 1), dtype=np.float64)
    phi[:, n_features] = base_margin(forest)
    offsets = forest["tree_offsets"]
    for t in range(offsets.shape[0] - 1):
        begin = int(offsets[t])
        phi[:, n_features] += mean[begin]
        node = np.full(n, begin, dtype=np.int64)
        while True:
            split = np.flatnonzero(forest["feature"][node] >= 0)
            if split.shape[0] == 0:
                break
            at = node[split]
            child = begin + _children(forest, at, rows, split)
            np.add.at(phi, (split, forest["feature"][at]), mean[child] - mean[at])
            node[split] = child
    return phi


# ---- forests for the awkward cases -----------------------------------------------------------------------------------
def awkward_forest():
    """Hand-written trees over 4 features: a stump, a single leaf, a feature split twice on one path (narrowing, and
    with `missing` on either side), a feature split three times on one path with another feature in between, and a
    repeated split whose interval is empty."""
    stump = tree([(1, 50.0, 1, 2, 2), 0.25, -0.5])
    leaf = tree([0.125])
    twice = tree([(0, 50.0, 1, 2, 1), (0, 20.0, 3, 4, 4), (2, 35.0, 5, 6, 5), -0.3, 0.2, 0.1, -0.15])
    thrice = tree([(0, 65.0, 1, 2, 2), (3, 35.0, 3, 4, 3), 0.4, (0, 35.0, 5, 6, 6), -0.2, -0.1, (0, 50.0, 7, 8, 7),
                   0.3, -0.25])
    empty = tree([(2, 20.0, 1, 2, 1), (2, 50.0, 3, 4, 4), 0.05, 0.35, (1, 50.0, 5, 6, 5), -0.45, 0.15])
    return from_trees([stump, leaf, twice, thrice, empty], base_margin=-0.4)


def enumerable_cases():
    """[(name, forest, cover, rows)]: forests small enough for shapley_brute_force (at most 8 features a tree, depth <= 6)
    that hold every awkward case: repeats (twice, three times), NaNs with `missing` on either side, a stump, a single
    leaf, covers of 1 against 10^6."""
    cases = []
    rng = np.random.RandomState(20)
    forest = awkward_forest()
    rows = small_rows(rng, 40, 4)
    counted = node_counts(forest, small_rows(rng, 500, 4)).astype(np.float64)
    cases.append(("awkward, counted cover + 1", forest, additive_cover(forest, counted + 1.0), rows))
    unequal = np.where(rng.rand(forest["feature"].shape[0]) < 0.5, 1.0, 1e6)
    cases.append(("awkward, covers 1 against 1e6", forest, additive_cover(forest, unequal), rows))
    two = from_trees([random_tree(rng, [0, 1], 6) for _ in range(3)], base_margin=0.3)
    rows = small_rows(rng, 30, 2)
    cases.append(("depth 6 on two features", two, additive_cover(two, rng.randint(1, 50, two["feature"].shape[0])), rows))
    cases.append(("depth 6 on two features, covers 1 against 1e6", two,
                  additive_cover(two, np.where(rng.rand(two["feature"].shape[0]) < 0.5, 1.0, 1e6)), rows))
    eight = from_trees([random_tree(rng, list(range(8)), 5) for _ in range(4)], base_margin=-1.0)
    rows = small_rows(rng, 24, 8)
    cases.append(("depth 5 on eight features", eight,
                  additive_cover(eight, rng.uniform(0.5, 20, eight["feature"].shape[0])), rows))
    return cases
