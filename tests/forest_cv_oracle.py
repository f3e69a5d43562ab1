"""The batched trainer's contract ("Cross-validation and tuning") composed from the functions of
forest_train_oracle: a model's held-out rows get (g, h) = (0, 0), its tree is grow_tree over ALL rows with those
gradients, every row is routed through it, and the held-out error is custom_error on the held-out rows."""
import numpy as np

import forest_train_oracle as oracle

DEFAULTS = dict(max_depth=5, eta=0.1, min_child_weight=1.0, reg_lambda=1.0, beta=5.0)


def zeroed(gh, fold, held_out):
    """gh with the rows of the held-out fold set to (0, 0); held_out = -1 holds nothing out."""
    out = np.array(gh, dtype=np.int64, copy=True)
    if held_out >= 0:
        out[np.asarray(fold) == held_out] = 0
    return out


def grow(node_bins, counts, gh, fold, model):
    """(heap tree, leaf per row) of one model's round from the gradients of ALL rows."""
    return oracle.grow_tree(node_bins, counts, zeroed(gh, fold, model.get("held_out", -1)), model["max_depth"],
                            model["eta"], model["min_child_weight"], model["reg_lambda"])


def grow_on_subset(node_bins, counts, gh, fold, model):
    """The same round on the training rows' columns of node_bins alone, with the same cuts."""
    keep = np.asarray(fold) != model.get("held_out", -1)
    return oracle.grow_tree(node_bins[:, keep], counts, np.asarray(gh)[keep], model["max_depth"], model["eta"],
                            model["min_child_weight"], model["reg_lambda"])


def same_tree(a, b):
    live = a["state"] != oracle.ABSENT
    return all(np.array_equal(a[key], b[key]) for key in ("state", "feature", "bin", "default_left")) and \
        np.array_equal(a["leaf"][live].view(np.uint32), b["leaf"][live].view(np.uint32))


def train(x, y, fold, model, rounds, max_bin=256):
    """Whole-oracle training of one model with NumPy's float32 sigmoid -> (trees, margins of all rows, errors)."""
    per_feature = oracle.cuts(x, max_bin)
    node_bins = oracle.bins(x, per_feature)
    counts = np.array([c.size for c in per_feature])
    leafsum = np.zeros(x.shape[0], np.float32)
    held = np.asarray(fold) == model.get("held_out", -1)
    trees, errors = [], []
    for _ in range(rounds):
        gh = oracle.gradients(oracle.sigmoid32(np.float32(0.0) + leafsum), y, model["beta"])
        tree, leaves = grow(node_bins, counts, gh, fold, model)
        leafsum = (leafsum + leaves).astype(np.float32)
        trees.append(tree)
        errors.append(oracle.custom_error(oracle.sigmoid32(np.float32(0.0) + leafsum[held]), y[held]))
    return trees, np.float32(0.0) + leafsum, errors
