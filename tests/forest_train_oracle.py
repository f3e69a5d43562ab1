"""NumPy restatement of the trainer's contract (DESIGN.md "Training"), written independently of train.py and
csrc/ds_train.hip: cuts, bins, quantized gradients, integer histograms, split choice with its tie order, leaves,
row routing and train.py's custom error.  Trees are heap-ordered like ds_trainer_step's: children of i are 2i + 1, 2i + 2,
state 0 absent, 2 split, 3 leaf."""
import numpy as np

QUANTUM = 2.0 ** 30
RT_EPS = 1e-6
MISSING = 255
ABSENT, SPLIT, LEAF = 0, 2, 3


def make_data(n, nf, seed):
    """Test features with NaNs, ties, a constant and an all-NaN column, +-0 and +-inf; labels from a noisy rule."""
    rng = np.random.RandomState(seed)
    x = rng.randn(n, nf).astype(np.float32)
    if nf > 1:
        x[:, 1] = np.round(x[:, 1] * 2)
    if nf > 2:
        x[rng.rand(n) < 0.2, 2] = np.nan
    if nf > 3:
        x[:, 3] = 7.0
    if nf > 4:
        x[:, 4] = np.nan
    if nf > 5:
        x[:, 5] = np.where(rng.rand(n) < 0.5, np.float32(-0.0), np.float32(0.0))
        x[rng.rand(n) < 0.05, 5] = np.inf
        x[rng.rand(n) < 0.05, 5] = -np.inf
    score = x[:, 0] + 0.5 * np.nan_to_num(x[:, min(2, nf - 1)]) + 0.3 * rng.randn(n)
    y = (score > 0.8).astype(np.float32)
    return x, y


# The trainer's limits (DESIGN.md "Training"): depth 8 and 96 features.  At levels 6 and 7 the histogram kernel
# builds 32 and 64 nodes in 16-node groups, and the split kernel gives level 7 a second workgroup of 64 nodes.
DEEP = dict(max_depth=8, eta=0.3, min_child_weight=0.5, reg_lambda=1.0)


def deep_wide_data(n=60000, seed=7):
    """make_data(n, 96, seed) with column 95 a bit-identical copy of column 0: its candidates tie with feature 0's in
    every node, in the last feature group, and must lose every tie."""
    x, y = make_data(n, 96, seed)
    x[:, 95] = x[:, 0]
    return x, y


def deep_paths(tree):
    """Counts of what a depth-8 heap tree reaches: (splits at heap ids 95..126, the children of level 5's second
    16-node group; splits at 191..254, the second 64-node workgroup of level 7; leaves at level 8, ids 255..510)."""
    state = tree["state"]
    return (int(np.count_nonzero(state[95:127] == SPLIT)), int(np.count_nonzero(state[191:255] == SPLIT)),
            int(np.count_nonzero(state[255:511] == LEAF)))


def cuts_of(column, max_bin=256):
    column = np.asarray(column, dtype=np.float32)
    present = column[column == column]
    values = np.sort(np.where(present == 0, np.float32(0.0), present))   # -0.0 -> +0.0
    if values.size == 0:
        return np.zeros(0, np.float32)
    distinct = np.unique(values)
    if distinct.size <= max_bin - 1:
        return distinct[1:].astype(np.float32)
    n = values.size
    chosen = []
    for j in range(1, max_bin - 1):
        value = values[(j * n) // (max_bin - 1)]
        if value != values[0] and (not chosen or chosen[-1] != value):
            chosen.append(value)
    return np.array(chosen, dtype=np.float32)


def cuts(features, max_bin=256):
    features = np.asarray(features, dtype=np.float32)
    return [cuts_of(features[:, f], max_bin) for f in range(features.shape[1])]


def bins(features, per_feature):
    """uint8[n_features, n]: searchsorted(cuts, x, 'right'), 255 for NaN."""
    features = np.asarray(features, dtype=np.float32)
    out = np.empty((features.shape[1], features.shape[0]), np.uint8)
    for f, c in enumerate(per_feature):
        x = features[:, f]
        b = np.searchsorted(c, x, side="right")
        out[f] = np.where(np.isnan(x), MISSING, b)
    return out


def sigmoid32(margin):
    margin = np.asarray(margin, dtype=np.float32)
    with np.errstate(over="ignore"):
        return (np.float32(1.0) / (np.float32(1.0) + np.exp(-margin))).astype(np.float32)


def gradients(p, y, beta=5.0):
    """int64[n, 2] = rint((g, h) * 2^30) of the weighted log loss at float32 probabilities p."""
    p = np.asarray(p, dtype=np.float32).astype(np.float64)
    y = np.asarray(y, dtype=np.float64)
    w = beta + y - beta * y
    g = p * w - y
    h = p * (1.0 - p) * w
    return np.stack([np.rint(g * QUANTUM), np.rint(h * QUANTUM)], axis=1).astype(np.int64)


def _exact_bincount(index, values, size):
    """Exact int64 sums of `values` per index (26-bit halves summed in float64, every partial sum below 2^53)."""
    values = np.asarray(values, dtype=np.int64)
    high, low = values >> 26, values & ((1 << 26) - 1)
    sum_high = np.rint(np.bincount(index, weights=high.astype(np.float64), minlength=size)).astype(np.int64)
    sum_low = np.rint(np.bincount(index, weights=low.astype(np.float64), minlength=size)).astype(np.int64)
    return (sum_high << 26) + sum_low


def histogram(node_bins, gh):
    """int64[n_features, 256, 2] of the rows given by node_bins (uint8[n_features, rows]) and gh (int64[rows, 2])."""
    nf, rows = node_bins.shape
    index = (np.arange(nf, dtype=np.int64)[:, None] * 256 + node_bins.astype(np.int64)).reshape(-1)
    out = np.empty((nf, 256, 2), np.int64)
    for k in range(2):
        out[:, :, k] = _exact_bincount(index, np.tile(gh[:, k], nf), nf * 256).reshape(nf, 256)
    return out


def best_split(hist, cut_counts, reg_lambda=1.0, min_child_weight=1.0):
    """(gain, feature, b, missing_left, (qGL, qHL)) of the best candidate, or None when there is none.
    Candidates: every feature f, b = 1 .. cut_counts[f], missing right then left; ties to the lower feature, then the
    lower b, then missing right (np.argmax returns the first maximum in that order)."""
    hist = np.asarray(hist, dtype=np.int64)
    nf = hist.shape[0]
    total = hist[0].sum(axis=0)
    prefix = np.cumsum(hist[:, :MISSING - 1, :], axis=1)        # prefix[f, b - 1] = sum of bins < b, b = 1 .. 254
    missing = hist[:, MISSING, :]
    left = np.stack([prefix, prefix + missing[:, None, :]], axis=2)   # [f, b - 1, missing_left, (g, h)]
    lam = float(reg_lambda)
    with np.errstate(divide="ignore", invalid="ignore"):
        GL, HL = left[..., 0] / QUANTUM, left[..., 1] / QUANTUM
        GR, HR = (total[0] - left[..., 0]) / QUANTUM, (total[1] - left[..., 1]) / QUANTUM
        G, H = total[0] / QUANTUM, total[1] / QUANTUM
        gain = GL * GL / (HL + lam) + GR * GR / (HR + lam) - G * G / (H + lam)
    b = np.arange(1, MISSING, dtype=np.int64)
    valid = (b[None, :] <= np.asarray(cut_counts)[:, None])[:, :, None] & (HL >= min_child_weight) & \
        (HR >= min_child_weight) & ~np.isnan(gain)
    gain = np.where(valid, gain, -np.inf)
    flat = int(np.argmax(gain))
    if not np.isfinite(gain.reshape(-1)[flat]):
        return None
    f, bm1, missing_left = np.unravel_index(flat, gain.shape)
    return (float(gain[f, bm1, missing_left]), int(f), int(bm1) + 1, int(missing_left),
            (int(left[f, bm1, missing_left, 0]), int(left[f, bm1, missing_left, 1])))


def leaf_value(qg, qh, reg_lambda, eta):
    return np.float32((-(qg / QUANTUM) / (qh / QUANTUM + reg_lambda)) * eta)


def grow_tree(node_bins, cut_counts, gh, max_depth=5, eta=0.1, min_child_weight=1.0, reg_lambda=1.0):
    """One tree from bins uint8[n_features, n] and quantized gradients int64[n, 2] -> (heap dict, leaf per row)."""
    slots = (2 << max_depth) - 1
    tree = dict(state=np.zeros(slots, np.int32), feature=np.full(slots, -1, np.int32), bin=np.zeros(slots, np.int32),
                default_left=np.zeros(slots, np.int32), leaf=np.zeros(slots, np.float32))
    node_of = np.zeros(node_bins.shape[1], np.int64)
    pending = {0: None}            # node -> its (qG, qH) when known from the parent's split
    for level in range(max_depth + 1):
        for node in range((1 << level) - 1, (2 << level) - 1):
            if node not in pending:
                continue
            rows = np.nonzero(node_of == node)[0]
            totals = pending[node]
            if level == max_depth:
                tree["state"][node] = LEAF
                tree["leaf"][node] = leaf_value(totals[0], totals[1], reg_lambda, eta)
                continue
            hist = histogram(node_bins[:, rows], gh[rows])
            G, H = (int(v) for v in hist[0].sum(axis=0))
            split = best_split(hist, cut_counts, reg_lambda, min_child_weight)
            if split is None or not split[0] > RT_EPS:
                tree["state"][node] = LEAF
                tree["leaf"][node] = leaf_value(G, H, reg_lambda, eta)
                continue
            _, f, b, missing_left, (lg, lh) = split
            tree["state"][node], tree["feature"][node], tree["bin"][node] = SPLIT, f, b
            tree["default_left"][node] = missing_left
            x = node_bins[f, rows]
            go_left = np.where(x == MISSING, bool(missing_left), x < b)
            node_of[rows] = np.where(go_left, 2 * node + 1, 2 * node + 2)
            pending[2 * node + 1] = (lg, lh)
            pending[2 * node + 2] = (G - lg, H - lh)
    return tree, tree["leaf"][route(tree, node_bins)]


def route(tree, node_bins):
    """The heap id of the leaf each row (column of node_bins) reaches."""
    node = np.zeros(node_bins.shape[1], np.int64)
    for _ in range(len(tree["state"]).bit_length()):
        state = tree["state"][node]
        moving = state == SPLIT
        if not moving.any():
            break
        x = node_bins[tree["feature"][node[moving]], np.nonzero(moving)[0]]
        left = np.where(x == MISSING, tree["default_left"][node[moving]] != 0, x < tree["bin"][node[moving]])
        node[moving] = np.where(left, 2 * node[moving] + 1, 2 * node[moving] + 2)
    return node


def custom_error(probabilities, target, threshold=0.9, penalty=5):
    """train.py fast_custom_error."""
    p = np.asarray(probabilities, dtype=np.float32).astype(np.float64)
    y = np.asarray(target)
    return int(y[p <= threshold].sum()) + penalty * int(np.count_nonzero(y[p > threshold] == 0))


def train(features, target, rounds, max_depth=5, eta=0.1, min_child_weight=1.0, reg_lambda=1.0, beta=5.0,
          max_bin=256):
    """Whole-oracle training with NumPy's float32 sigmoid (timing reference; margins float32[n] and heap trees)."""
    per_feature = cuts(features, max_bin)
    node_bins = bins(features, per_feature)
    counts = np.array([c.size for c in per_feature])
    leafsum = np.zeros(node_bins.shape[1], np.float32)
    trees = []
    for _ in range(rounds):
        gh = gradients(sigmoid32(np.float32(0.0) + leafsum), target, beta)
        tree, leaves = grow_tree(node_bins, counts, gh, max_depth, eta, min_child_weight, reg_lambda)
        leafsum = (leafsum + leaves).astype(np.float32)
        trees.append(tree)
    return trees, np.float32(0.0) + leafsum
