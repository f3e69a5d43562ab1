"""NumPy restatement of the trainer's sample-weight rule ("Sample weights") on top of
forest_train_oracle, written independently of csrc/ds_train.h: row r of weight s_r (a float32, widened to float64)
carries

    g = (p*w - y) * s_r,  h = (p*(1 - p)*w) * s_r,  gh[r] = (rint(g * 2^30), rint(h * 2^30))

with p the float32 probability, y the label, w = beta + y - beta*y and the parenthesised factors computed exactly as
forest_train_oracle.gradients computes g and h.  Everything after the gradients is forest_train_oracle's."""
import numpy as np

import forest_train_oracle as oracle

# what every weight test draws from: non-dyadic values, zeros and a large one
WEIGHT_VALUES = np.array([0, 0.1, 1 / 3, 0.25, 1, 2, 3.5, 1000], np.float64)


def draw_weights(n, seed):
    """float32[n] drawn from WEIGHT_VALUES, with at least one positive weight."""
    weights = WEIGHT_VALUES[np.random.RandomState(seed).randint(0, WEIGHT_VALUES.shape[0], n)].astype(np.float32)
    if not (weights > 0).any():
        weights[0] = np.float32(1 / 3)
    return weights


def gradients(p, y, s, beta=5.0):
    """int64[n, 2] = rint((g, h) * 2^30) of the weighted log loss at float32 probabilities p with float32 weights s."""
    p = np.asarray(p, dtype=np.float32).astype(np.float64)
    y = np.asarray(y, dtype=np.float64)
    s = np.asarray(s, dtype=np.float32).astype(np.float64)
    w = beta + y - beta * y
    g = (p * w - y) * s
    h = (p * (1.0 - p) * w) * s
    return np.stack([np.rint(g * oracle.QUANTUM), np.rint(h * oracle.QUANTUM)], axis=1).astype(np.int64)


def train(features, target, weights, rounds, max_depth=5, eta=0.1, min_child_weight=1.0, reg_lambda=1.0, beta=5.0,
          max_bin=256):
    """forest_train_oracle.train with sample weights -> (trees, margins float32[n], the cuts per feature, the
    quantized gradients of every round)."""
    per_feature = oracle.cuts(features, max_bin)
    node_bins = oracle.bins(features, per_feature)
    counts = np.array([c.size for c in per_feature])
    leafsum = np.zeros(node_bins.shape[1], np.float32)
    trees, every_gh = [], []
    for _ in range(rounds):
        gh = gradients(oracle.sigmoid32(np.float32(0.0) + leafsum), target, weights, beta)
        tree, leaves = oracle.grow_tree(node_bins, counts, gh, max_depth, eta, min_child_weight, reg_lambda)
        leafsum = (leafsum + leaves).astype(np.float32)
        trees.append(tree)
        every_gh.append(gh)
    return trees, np.float32(0.0) + leafsum, per_feature, every_gh


def stacked(x, y, weights, seed):
    """The matrix stacked on a copy of itself whose rows carry flipped labels and weight 0, all rows permuted ->
    (features, labels, weights, where: the position of every original row).  A row of weight 0 trains nothing and a
    copy adds no value to any column, so this matrix grows the trees of (x, y, weights) alone."""
    n = x.shape[0]
    order = np.random.RandomState(seed).permutation(2 * n)
    features = np.concatenate((x, x))[order]
    labels = np.concatenate((y, 1 - y)).astype(np.float32)[order]
    both = np.concatenate((weights, np.zeros(n, np.float32))).astype(np.float32)[order]
    where = np.empty(2 * n, np.int64)
    where[order] = np.arange(2 * n)
    return features, labels, both, where[:n]


def same_tree(a, b):
    """Heap trees equal in structure and in the bits of their leaves."""
    live = a["state"] != oracle.ABSENT
    return all(np.array_equal(a[key], b[key]) for key in ("state", "feature", "bin", "default_left")) and \
        np.array_equal(a["leaf"][live].view(np.uint32), b["leaf"][live].view(np.uint32))
