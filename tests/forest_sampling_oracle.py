"""NumPy restatement of the trainer's subsampling rule ("Subsampling") on top of
forest_train_oracle and forest_cv_oracle, written independently of csrc/ds_train.h: the splitmix64 stream of (seed,
purpose, index) in pure Python and in NumPy uint64, the row mask of a round, the feature set of a tree and of each of
its levels, a grow_tree that takes a per-level feature mask, and whole-model training with the four parameters."""
import math

import numpy as np

import forest_cv_oracle as cv_oracle
import forest_train_oracle as oracle

MASK = (1 << 64) - 1
PURPOSE_ROW, PURPOSE_TREE, PURPOSE_LEVEL = 3, 4, 5     # include/doppel_amd.h DS_SAMPLE_PURPOSE_*
DEFAULTS = dict(cv_oracle.DEFAULTS, subsample=1.0, colsample_bytree=1.0, colsample_bylevel=1.0, sample_seed=0)


def key(seed, purpose, index):
    """The first kept output of the stream of (seed, purpose, index), in Python integers: the state formula, two
    outputs thrown away, the third returned."""
    state = (seed * 0x9e3779b97f4a7c15 + index * 0xd1342543de82ef95 + purpose * 0xaf251af3b0f025b5) & MASK
    for _ in range(3):
        state = (state + 0x9e3779b97f4a7c15) & MASK
        z = state
        z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & MASK
        z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & MASK
        z ^= z >> 31
    return z


def keys(seed, purpose, indexes):
    """key() of every index of an array, in NumPy uint64 (arithmetic modulo 2^64)."""
    u = np.uint64
    with np.errstate(over="ignore"):
        start = u((seed * 0x9e3779b97f4a7c15 + purpose * 0xaf251af3b0f025b5 + 3 * 0x9e3779b97f4a7c15) & MASK)
        z = np.asarray(indexes).astype(np.uint64) * u(0xd1342543de82ef95) + start
        z = (z ^ (z >> u(30))) * u(0xbf58476d1ce4e5b9)
        z = (z ^ (z >> u(27))) * u(0x94d049bb133111eb)
        return z ^ (z >> u(31))


def row_mask(seed, tree, n_rows, subsample):
    """bool[n_rows]: training row r (its number among the rows that train) trains in the model's tree `tree`."""
    if subsample == 1:
        return np.ones(n_rows, bool)
    x = keys(seed, PURPOSE_ROW, np.uint64(tree << 32) | np.arange(n_rows, dtype=np.uint64))
    return (x >> np.uint64(11)).astype(np.float64) * 2.0 ** -53 < subsample


def set_size(fraction, available):
    return max(1, int(math.floor(fraction * available)))


def _smallest(candidates, their_keys, count):
    """The `count` candidates with the smallest key, ties to the lower feature (candidates ascend; a stable sort)."""
    order = np.argsort(their_keys, kind="stable")
    return np.sort(candidates[order[:count]])


def tree_set(seed, tree, n_features, colsample_bytree):
    """The ascending feature numbers of the tree's set."""
    features = np.arange(n_features)
    if colsample_bytree == 1:
        return features
    return _smallest(features, keys(seed, PURPOSE_TREE, np.uint64(tree << 32) | features.astype(np.uint64)),
                     set_size(colsample_bytree, n_features))


def level_set(seed, tree, level, of_tree, colsample_bylevel):
    """The features OF THE TREE'S SET that level `level` may split on."""
    of_tree = np.asarray(of_tree)
    if colsample_bylevel == 1:
        return of_tree
    index = np.uint64((tree << 32) | (level << 8)) | of_tree.astype(np.uint64)
    return _smallest(of_tree, keys(seed, PURPOSE_LEVEL, index), set_size(colsample_bylevel, of_tree.size))


def level_masks(seed, tree, n_features, max_depth, colsample_bytree, colsample_bylevel):
    """bool[max_depth, n_features]: the level sets of one tree."""
    of_tree = tree_set(seed, tree, n_features, colsample_bytree)
    out = np.zeros((max_depth, n_features), bool)
    for level in range(max_depth):
        out[level, level_set(seed, tree, level, of_tree, colsample_bylevel)] = True
    return out


def grow_tree(node_bins, cut_counts, gh, masks, max_depth=5, eta=0.1, min_child_weight=1.0, reg_lambda=1.0):
    """forest_train_oracle.grow_tree with masks[level, f] false = feature f offers no candidate at that level (as a
    feature without cuts).  Every node's histogram is summed from its rows: no parent - sibling shortcut to get wrong."""
    slots = (2 << max_depth) - 1
    tree = dict(state=np.zeros(slots, np.int32), feature=np.full(slots, -1, np.int32), bin=np.zeros(slots, np.int32),
                default_left=np.zeros(slots, np.int32), leaf=np.zeros(slots, np.float32))
    node_of = np.zeros(node_bins.shape[1], np.int64)
    pending = {0: None}
    cut_counts = np.asarray(cut_counts)
    for level in range(max_depth + 1):
        for node in range((1 << level) - 1, (2 << level) - 1):
            if node not in pending:
                continue
            rows = np.nonzero(node_of == node)[0]
            totals = pending[node]
            if level == max_depth:
                tree["state"][node] = oracle.LEAF
                tree["leaf"][node] = oracle.leaf_value(totals[0], totals[1], reg_lambda, eta)
                continue
            hist = oracle.histogram(node_bins[:, rows], gh[rows])
            G, H = (int(v) for v in hist[0].sum(axis=0))
            split = oracle.best_split(hist, np.where(masks[level], cut_counts, 0), reg_lambda, min_child_weight)
            if split is None or not split[0] > oracle.RT_EPS:
                tree["state"][node] = oracle.LEAF
                tree["leaf"][node] = oracle.leaf_value(G, H, reg_lambda, eta)
                continue
            _, f, b, missing_left, (lg, lh) = split
            tree["state"][node], tree["feature"][node], tree["bin"][node] = oracle.SPLIT, f, b
            tree["default_left"][node] = missing_left
            x = node_bins[f, rows]
            go_left = np.where(x == oracle.MISSING, bool(missing_left), x < b)
            node_of[rows] = np.where(go_left, 2 * node + 1, 2 * node + 2)
            pending[2 * node + 1] = (lg, lh)
            pending[2 * node + 2] = (G - lg, H - lh)
    return tree, tree["leaf"][oracle.route(tree, node_bins)]


class Booster:
    """One model, grown round by round over ALL rows of a matrix.  Rows of fold `held_out` never train; of the others,
    numbered 0, 1, .. in row order, round t trains those of row_mask(sample_seed, t, ..).  step(probabilities) takes the
    float32 probabilities the gradients are to be taken at (default: NumPy's sigmoid of its own margins), so that a test
    can hand in the device's, whose expf may differ from NumPy's in the last bits."""

    def __init__(self, features, target, parameters=None, fold=None, held_out=-1, per_feature=None, max_bin=256):
        self.parameters = dict(DEFAULTS, **(parameters or {}))
        features = np.asarray(features, np.float32)
        self.y = np.asarray(target)
        self.per_feature = oracle.cuts(features, max_bin) if per_feature is None else per_feature
        self.node_bins = oracle.bins(features, self.per_feature)
        self.counts = np.array([c.size for c in self.per_feature])
        n = features.shape[0]
        self.trains = np.ones(n, bool) if fold is None or held_out < 0 else np.asarray(fold) != held_out
        self.leafsum = np.zeros(n, np.float32)
        self.trees, self.row_masks, self.masks = [], [], []

    def margins(self):
        return np.float32(0.0) + self.leafsum

    def step(self, probabilities=None):
        """One round -> (tree, the quantised gradients as trained: (0, 0) in rows that do not train)."""
        q = self.parameters
        t = len(self.trees)
        p = oracle.sigmoid32(self.margins()) if probabilities is None else probabilities
        drawn = np.zeros(self.trains.shape[0], bool)
        drawn[self.trains] = row_mask(q["sample_seed"], t, int(self.trains.sum()), q["subsample"])
        gh = oracle.gradients(p, self.y, q["beta"])
        gh[~drawn] = 0
        masks = level_masks(q["sample_seed"], t, self.node_bins.shape[0], q["max_depth"], q["colsample_bytree"],
                            q["colsample_bylevel"])
        tree, leaves = grow_tree(self.node_bins, self.counts, gh, masks, q["max_depth"], q["eta"],
                                 q["min_child_weight"], q["reg_lambda"])
        self.leafsum = (self.leafsum + leaves).astype(np.float32)
        self.trees.append(tree)
        self.row_masks.append(drawn)
        self.masks.append(masks)
        return tree, gh


def train(features, target, rounds, eval_features=None, eval_target=None, fold=None, held_out=-1, max_bin=256,
          **parameters):
    """Whole-oracle training with NumPy's float32 sigmoid -> (trees, margins of ALL rows, errors): the errors are
    train.py's custom error of the evaluation set after every round, or of the held-out fold, or absent."""
    booster = Booster(features, target, parameters, fold, held_out, max_bin=max_bin)
    eval_bins = None if eval_features is None else oracle.bins(eval_features, booster.per_feature)
    eval_sum = None if eval_features is None else np.zeros(eval_bins.shape[1], np.float32)
    errors = []
    for _ in range(rounds):
        tree, _ = booster.step()
        if eval_bins is not None:
            eval_sum = (eval_sum + tree["leaf"][oracle.route(tree, eval_bins)]).astype(np.float32)
            errors.append(oracle.custom_error(oracle.sigmoid32(np.float32(0.0) + eval_sum), eval_target))
        elif not booster.trains.all():
            held = ~booster.trains
            errors.append(oracle.custom_error(oracle.sigmoid32(booster.margins()[held]), booster.y[held]))
    return booster.trees, booster.margins(), errors
