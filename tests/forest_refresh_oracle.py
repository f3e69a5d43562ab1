"""NumPy restatement of the refresh rule ("Refreshing a model"), written from the rule and not from
csrc/ds_refresh.hip: the model's flat arrays, raw float32 features, and per tree the float32 probabilities it is
HANDED (the device's expf is not NumPy's, so a GPU test passes the device's `trace`; None takes NumPy's sigmoid).  Sums
are the exact integer sums of forest_train_oracle._exact_bincount."""
import numpy as np

from forest_train_oracle import QUANTUM, _exact_bincount, custom_error, leaf_value, sigmoid32


def walk(arrays, tree, features):
    """int64[n]: the node (in the model's node order) of the leaf every raw row reaches in tree `tree`."""
    features = np.asarray(features, dtype=np.float32)
    root = int(arrays["tree_offsets"][tree])
    node = np.zeros(features.shape[0], np.int64)
    rows = np.arange(features.shape[0])
    while True:
        split = arrays["feature"][root + node]
        moving = split >= 0
        if not moving.any():
            return root + node
        at = root + node[moving]
        x = features[rows[moving], split[moving]]
        with np.errstate(invalid="ignore"):
            below = x < arrays["threshold"][at]
        node[moving] = np.where(np.isnan(x), arrays["missing"][at], np.where(below, arrays["yes"][at], arrays["no"][at]))


def gradients(p, y, beta, weights=None):
    """int64[n, 2] = rint((g, h) * 2^30): the weight widened to double is the last factor."""
    p = np.asarray(p, dtype=np.float32).astype(np.float64)
    y = np.asarray(y, dtype=np.float64)
    s = np.ones(y.shape[0]) if weights is None else np.asarray(weights, dtype=np.float32).astype(np.float64)
    w = beta + y - beta * y
    g = (p * w - y) * s
    h = (p * (1.0 - p) * w) * s
    return np.stack([np.rint(g * QUANTUM), np.rint(h * QUANTUM)], axis=1).astype(np.int64)


def inner_sums(arrays, node_sums):
    """node_sums with every split node set to the sum of its two children (children come after their parent)."""
    out = np.array(node_sums, dtype=np.int64)
    offsets = arrays["tree_offsets"]
    for t in range(offsets.shape[0] - 1):
        begin, end = int(offsets[t]), int(offsets[t + 1])
        for i in range(end - 1, begin - 1, -1):
            if arrays["feature"][i] >= 0:
                out[i] = out[begin + arrays["yes"][i]] + out[begin + arrays["no"][i]]
    return out


def refresh(arrays, features, target, probabilities=None, weights=None, eta=0.1, reg_lambda=1.0, beta=5.0,
            refresh_leaf=True, eval_features=None, eval_target=None):
    """-> dict(leaves float32[n_nodes] (a split keeps its threshold), node_sums int64[n_nodes, 2], margins float32[n],
    empty_leaves, before float32[n_trees, n]: the margins each tree's probabilities belong to, and with an evaluation
    set initial_error, history and eval_margins float32[n_trees + 1, n_eval]: the margins initial_error and every entry of
    history were counted at)."""
    features = np.asarray(features, dtype=np.float32)
    n, n_nodes = features.shape[0], arrays["feature"].shape[0]
    n_trees = arrays["tree_offsets"].shape[0] - 1
    base = np.float32(arrays["base_margin"])
    values = arrays["threshold"].astype(np.float32).copy()
    work = dict(arrays, threshold=values)
    sums = np.zeros((n_nodes, 2), np.int64)
    leafsum = np.zeros(n, np.float32)
    before = np.zeros((n_trees, n), np.float32)
    out = {}
    if eval_features is not None:
        eval_features = np.asarray(eval_features, dtype=np.float32)
        old = np.zeros(eval_features.shape[0], np.float32)
        for t in range(n_trees):
            old = (old + arrays["threshold"][walk(arrays, t, eval_features)]).astype(np.float32)
        out["initial_error"] = custom_error(sigmoid32(base + old), eval_target)
        eval_leafsum, history, prefix_margins = np.zeros(eval_features.shape[0], np.float32), [], [base + old]
    for t in range(n_trees):
        before[t] = base + leafsum
        if n:
            p = sigmoid32(before[t]) if probabilities is None else probabilities[t]
            gh = gradients(p, target, beta, weights)
            leaf = walk(work, t, features)
            for k in range(2):
                sums[:, k] += _exact_bincount(leaf, gh[:, k], n_nodes)
            if refresh_leaf:
                begin, end = int(arrays["tree_offsets"][t]), int(arrays["tree_offsets"][t + 1])
                for i in range(begin, end):
                    if arrays["feature"][i] < 0 and sums[i, 1] > 0:
                        values[i] = leaf_value(int(sums[i, 0]), int(sums[i, 1]), reg_lambda, eta)
            leafsum = (leafsum + values[leaf]).astype(np.float32)
        if eval_features is not None:
            eval_leafsum = (eval_leafsum + values[walk(work, t, eval_features)]).astype(np.float32)
            history.append(custom_error(sigmoid32(base + eval_leafsum), eval_target))
            prefix_margins.append(base + eval_leafsum)
    leaves = arrays["feature"] < 0
    out.update(leaves=values, node_sums=inner_sums(arrays, sums), margins=(base + leafsum).astype(np.float32),
               empty_leaves=int(np.count_nonzero(sums[leaves, 1] == 0)), before=before)
    if eval_features is not None:
        out.update(history=history, eval_margins=np.stack(prefix_margins).astype(np.float32))
    return out
