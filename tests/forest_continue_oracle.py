"""NumPy restatement of "Continuing from a model"  on top of forest_train_oracle and
forest_sampling_oracle, written independently of csrc/ds_train.hip and csrc/ds_forest.h: a plain tree walk of a forest
over RAW float32 features (the seed of a trainer's leaf sums), a Booster that starts from such a seed and numbers its
trees on from the forest's, and the conversion of the oracle's heap trees into the flat arrays of a forest."""
import numpy as np

import forest_sampling_oracle as sampling
import forest_train_oracle as oracle

TREE_KEYS = ("feature", "threshold", "yes", "no", "missing")


def leaf_sums(arrays, features, events=None):
    """float32[n]: per row the leaves it reaches in every tree of the flat arrays (feature < 0: a leaf whose value is
    `threshold`; children tree-relative), summed from zero in tree order in float32.  A NaN follows `missing`, any
    other value v follows `yes` when v < threshold and `no` otherwise (so -0.0 < 0.0 is false).
    events (a dict) counts what the walk met: "nan" decisions taken by `missing`, "yes" and "no" decisions."""
    features = np.asarray(features, dtype=np.float32)
    offsets = np.asarray(arrays["tree_offsets"])
    total = np.zeros(features.shape[0], np.float32)
    rows = np.arange(features.shape[0])
    for t in range(offsets.shape[0] - 1):
        root = int(offsets[t])
        node = np.full(features.shape[0], root, np.int64)
        while True:
            moving = np.nonzero(arrays["feature"][node] >= 0)[0]
            if moving.size == 0:
                break
            at = node[moving]
            value = features[rows[moving], arrays["feature"][at]]
            is_nan = np.isnan(value)
            with np.errstate(invalid="ignore"):
                below = value < arrays["threshold"][at]
            child = np.where(is_nan, arrays["missing"][at], np.where(below, arrays["yes"][at], arrays["no"][at]))
            if events is not None:
                events["nan"] = events.get("nan", 0) + int(is_nan.sum())
                events["yes"] = events.get("yes", 0) + int((~is_nan & below).sum())
                events["no"] = events.get("no", 0) + int((~is_nan & ~below).sum())
            node[moving] = root + child
        total = (total + arrays["threshold"][node]).astype(np.float32)
    return total


def flat_tree(tree, per_feature):
    """One heap tree of the oracle -> the per-tree arrays of a forest, nodes in breadth-first order (children after
    their parent): a split on (feature f, bin b) becomes `x < cuts[f][b - 1]`, missing to the default side."""
    order, ids = [0], {0: 0}
    for node in order:
        if tree["state"][node] == oracle.SPLIT:
            for child in (2 * node + 1, 2 * node + 2):
                ids[child] = len(order)
                order.append(child)
    out = dict(feature=np.full(len(order), -1, np.int32), threshold=np.zeros(len(order), np.float32),
               yes=np.zeros(len(order), np.int32), no=np.zeros(len(order), np.int32),
               missing=np.zeros(len(order), np.int32))
    for i, node in enumerate(order):
        if tree["state"][node] == oracle.SPLIT:
            f, b = int(tree["feature"][node]), int(tree["bin"][node])
            out["feature"][i], out["threshold"][i] = f, per_feature[f][b - 1]
            out["yes"][i], out["no"][i] = ids[2 * node + 1], ids[2 * node + 2]
            out["missing"][i] = out["yes"][i] if tree["default_left"][node] else out["no"][i]
        else:
            assert tree["state"][node] == oracle.LEAF
            out["threshold"][i] = tree["leaf"][node]
    return out


def flat_forest(trees):
    """Per-tree arrays -> the flat arrays of a forest with base margin 0."""
    offsets = np.zeros(len(trees) + 1, np.int64)
    offsets[1:] = np.cumsum([tree["feature"].shape[0] for tree in trees])
    dtypes = dict(feature=np.int32, threshold=np.float32, yes=np.int32, no=np.int32, missing=np.int32)
    out = {key: np.concatenate([tree[key] for tree in trees]).astype(dtypes[key]) if trees else np.zeros(0, dtypes[key])
           for key in TREE_KEYS}
    return dict(out, tree_offsets=offsets, base_margin=0.0)


def random_forest(n_trees, depth, n_features, seed, scale=1.0):
    """A hand-built forest: `n_trees` complete trees of `depth` levels of splits on random features at random
    thresholds (normal, times `scale`; some exactly 0.0, which -0.0 is NOT below), `missing` to either side at random,
    leaves normal / 10."""
    rng = np.random.RandomState(seed)
    trees = []
    for _ in range(n_trees):
        inner, size = (1 << depth) - 1, (2 << depth) - 1
        ids = np.arange(size)
        tree = dict(feature=np.full(size, -1, np.int32), threshold=(rng.randn(size) / 10).astype(np.float32),
                    yes=np.zeros(size, np.int32), no=np.zeros(size, np.int32), missing=np.zeros(size, np.int32))
        tree["feature"][:inner] = rng.randint(0, n_features, inner)
        thresholds = (rng.randn(inner) * scale).astype(np.float32)
        thresholds[rng.rand(inner) < 0.15] = 0.0
        tree["threshold"][:inner] = thresholds
        tree["yes"][:inner], tree["no"][:inner] = 2 * ids[:inner] + 1, 2 * ids[:inner] + 2
        tree["missing"][:inner] = np.where(rng.rand(inner) < 0.5, tree["yes"][:inner], tree["no"][:inner])
        trees.append(tree)
    return trees


class ContinueBooster(sampling.Booster):
    """forest_sampling_oracle.Booster that continues from a forest (flat arrays, base margin 0): its leaf sums start
    at leaf_sums(forest, RAW features) -- of ALL rows, held-out ones included -- and its first tree has the number
    of the forest's trees, which indexes the sampling streams.  `trees` holds the NEW trees."""

    def __init__(self, features, target, init_arrays, parameters=None, fold=None, held_out=-1, per_feature=None,
                 max_bin=256):
        super().__init__(features, target, parameters, fold, held_out, per_feature, max_bin)
        assert init_arrays["base_margin"] == 0.0
        self.first_tree = int(np.asarray(init_arrays["tree_offsets"]).shape[0]) - 1
        self.leafsum = leaf_sums(init_arrays, features)

    def step(self, probabilities=None):
        q = self.parameters
        t = self.first_tree + len(self.trees)
        p = oracle.sigmoid32(self.margins()) if probabilities is None else probabilities
        drawn = np.zeros(self.trains.shape[0], bool)
        drawn[self.trains] = sampling.row_mask(q["sample_seed"], t, int(self.trains.sum()), q["subsample"])
        gh = oracle.gradients(p, self.y, q["beta"])
        gh[~drawn] = 0
        masks = sampling.level_masks(q["sample_seed"], t, self.node_bins.shape[0], q["max_depth"],
                                     q["colsample_bytree"], q["colsample_bylevel"])
        tree, leaves = sampling.grow_tree(self.node_bins, self.counts, gh, masks, q["max_depth"], q["eta"],
                                          q["min_child_weight"], q["reg_lambda"])
        self.leafsum = (self.leafsum + leaves).astype(np.float32)
        self.trees.append(tree)
        self.row_masks.append(drawn)
        self.masks.append(masks)
        return tree, gh


def error_of(leafsum, target):
    """train.py's custom error at margins 0 + leafsum, with NumPy's float32 sigmoid."""
    return oracle.custom_error(oracle.sigmoid32(np.float32(0.0) + leafsum), target)


def train(features, target, rounds, init_arrays=None, eval_features=None, eval_target=None, max_bin=256, **parameters):
    """Whole-oracle training with NumPy's float32 sigmoid, from zero or (init_arrays) continued from a forest ->
    dict(trees: the new heap trees, flat: their per-tree arrays, margins, eval_margins, errors per new round,
    initial_error: that of the seeded evaluation margins)."""
    if init_arrays is None:
        init_arrays = flat_forest([])
    booster = ContinueBooster(features, target, init_arrays, parameters, max_bin=max_bin)
    out = dict(errors=[], initial_error=None, eval_margins=None)
    if eval_features is not None:
        eval_bins = oracle.bins(eval_features, booster.per_feature)
        eval_sum = leaf_sums(init_arrays, eval_features)
        out["initial_error"] = error_of(eval_sum, eval_target)
    for _ in range(rounds):
        tree, _ = booster.step()
        if eval_features is not None:
            eval_sum = (eval_sum + tree["leaf"][oracle.route(tree, eval_bins)]).astype(np.float32)
            out["errors"].append(error_of(eval_sum, eval_target))
    if eval_features is not None:
        out["eval_margins"] = np.float32(0.0) + eval_sum
    out["trees"] = booster.trees
    out["flat"] = [flat_tree(tree, booster.per_feature) for tree in booster.trees]
    out["margins"] = booster.margins()
    return out
