"""NumPy restatement of the trainer's monotone-constraint rule ("Monotone constraints") on top
of forest_train_oracle, written from that text and independently of csrc/ds_train.h.  Cuts, bins, gradients, histogram
and route are forest_train_oracle's; the split choice, the bounds and the leaves are restated here, all in float64 and
in the section's operation order:

    w(G, H) = -G / (H + lambda),  w* = min(max(w, lo), hi)
    T(G, H) = G * G / (H + lambda)                                   while lo <= w <= hi
            = -(((2.0 * G) * w*) + (((H + lambda) * w*) * w*))       otherwise
    gain    = T(GL, HL) + T(GR, HR) - T(G, H)                        all three under the NODE's bounds
    a candidate on feature f that passed min_child_weight is rejected when c[f] > 0 and wL* > wR*, or c[f] < 0 and
    wL* < wR*; children of the winner: mid = (wL* + wR*) / 2.0, c[f] > 0: left [lo, mid], right [mid, hi];
    c[f] < 0: left [mid, hi], right [lo, mid]; c[f] == 0: both [lo, hi]; leaf = float32(w* * eta) under its own bounds.

Besides the trees it counts, per tree, the candidates the constraints rejected, the leaves that were clamped and the
splits that violate the constraints (violations, the same count as ForestModel.monotone_violations)."""
import numpy as np

import forest_train_oracle as oracle

# n, features, depth, reg_lambda, min_child_weight, eta: the cases of the CPU and the GPU tests
CASES = [(9, 6, 3, 1.0, 0.0, 0.3), (63, 6, 2, 0.0, 0.5, 0.3), (64, 10, 4, 1.0, 1.0, 0.1), (65, 6, 1, 1.0, 1.0, 0.3),
         (300, 10, 5, 1.0, 1.0, 0.3), (1000, 10, 6, 1.0, 0.5, 0.3)]
CLAMPING = (9, 63, 300, 1000)        # the cases (by n) that must clamp at least one leaf
ONE_ROW = (1, 3, 1, 1.0, 1.0, 0.1)
ROUNDS = 4


def case_constraints(nf):
    """make_data's label rises with column 0, so -1 there is the wrong way; columns 1 and 2 are constrained upwards."""
    c = np.zeros(nf, np.int8)
    c[0] = -1
    c[1:3] = 1
    return c


def idle_constraints(nf):
    """Constraints only on make_data's constant column 3 and all-NaN column 4, which offer no boundary: nothing binds."""
    c = np.zeros(nf, np.int8)
    c[3], c[4] = 1, -1
    return c


def bounded(G, H, lam, lo, hi):
    """(w*, T, clamped) of sums (G, H) under bounds [lo, hi]; scalars or arrays."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        w = -G / (H + lam)
        star = np.minimum(np.maximum(w, lo), hi)
        inside = (lo <= w) & (w <= hi)
        term = np.where(inside, G * G / (H + lam), -(((2.0 * G) * star) + (((H + lam) * star) * star)))
    return star, term, ~inside


def best_split(hist, cut_counts, constraints, lo, hi, reg_lambda=1.0, min_child_weight=1.0):
    """((gain, feature, b, missing_left, (qGL, qHL)) or None, the number of candidates rejected by the constraints).
    The candidate order and the tie order are forest_train_oracle.best_split's: np.argmax returns the first maximum over
    [feature, b, missing right then left]."""
    hist = np.asarray(hist, dtype=np.int64)
    total = hist[0].sum(axis=0)
    prefix = np.cumsum(hist[:, :oracle.MISSING - 1, :], axis=1)
    missing = hist[:, oracle.MISSING, :]
    left = np.stack([prefix, prefix + missing[:, None, :]], axis=2)      # [f, b - 1, missing_left, (g, h)]
    lam = float(reg_lambda)
    GL, HL = left[..., 0] / oracle.QUANTUM, left[..., 1] / oracle.QUANTUM
    GR, HR = (total[0] - left[..., 0]) / oracle.QUANTUM, (total[1] - left[..., 1]) / oracle.QUANTUM
    G, H = total[0] / oracle.QUANTUM, total[1] / oracle.QUANTUM
    wl, tl, _ = bounded(GL, HL, lam, lo, hi)
    wr, tr, _ = bounded(GR, HR, lam, lo, hi)
    _, tp, _ = bounded(G, H, lam, lo, hi)
    gain = tl + tr - tp
    b = np.arange(1, oracle.MISSING, dtype=np.int64)
    heavy = (b[None, :] <= np.asarray(cut_counts)[:, None])[:, :, None] & (HL >= min_child_weight) & \
        (HR >= min_child_weight)
    sign = np.asarray(constraints)[:, None, None]
    wrong = ((sign > 0) & (wl > wr)) | ((sign < 0) & (wl < wr))
    rejected = int(np.count_nonzero(heavy & wrong))
    gain = np.where(heavy & ~wrong & ~np.isnan(gain), gain, -np.inf)
    flat = int(np.argmax(gain))
    if not np.isfinite(gain.reshape(-1)[flat]):
        return None, rejected
    f, bm1, missing_left = np.unravel_index(flat, gain.shape)
    return (float(gain[f, bm1, missing_left]), int(f), int(bm1) + 1, int(missing_left),
            (int(left[f, bm1, missing_left, 0]), int(left[f, bm1, missing_left, 1]))), rejected


def leaf_value(qg, qh, reg_lambda, eta, lo, hi):
    """(float32(w* * eta), whether the weight was clamped)."""
    star, _, clamped = bounded(qg / oracle.QUANTUM, qh / oracle.QUANTUM, float(reg_lambda), lo, hi)
    return np.float32(star * eta), bool(clamped)


def grow_tree(node_bins, cut_counts, gh, constraints, max_depth=5, eta=0.1, min_child_weight=1.0, reg_lambda=1.0):
    """One tree under the constraints from bins uint8[n_features, n] and quantized gradients int64[n, 2] ->
    (heap dict, leaf per row, dict(rejected, clamped, rejected_at: {heap id: its rejected candidates})).  The heap dict
    also carries `lo` and `hi` of every node."""
    slots = (2 << max_depth) - 1
    tree = dict(state=np.zeros(slots, np.int32), feature=np.full(slots, -1, np.int32), bin=np.zeros(slots, np.int32),
                default_left=np.zeros(slots, np.int32), leaf=np.zeros(slots, np.float32),
                lo=np.full(slots, -np.inf), hi=np.full(slots, np.inf))
    counts = dict(rejected=0, clamped=0, rejected_at={})
    node_of = np.zeros(node_bins.shape[1], np.int64)
    pending = {0: None}
    lam = float(reg_lambda)

    def make_leaf(node, qg, qh):
        tree["state"][node] = oracle.LEAF
        tree["leaf"][node], clamped = leaf_value(qg, qh, lam, eta, tree["lo"][node], tree["hi"][node])
        counts["clamped"] += int(clamped)

    for level in range(max_depth + 1):
        for node in range((1 << level) - 1, (2 << level) - 1):
            if node not in pending:
                continue
            if level == max_depth:
                make_leaf(node, *pending[node])
                continue
            rows = np.nonzero(node_of == node)[0]
            hist = oracle.histogram(node_bins[:, rows], gh[rows])
            G, H = (int(v) for v in hist[0].sum(axis=0))
            lo, hi = tree["lo"][node], tree["hi"][node]
            split, rejected = best_split(hist, cut_counts, constraints, lo, hi, lam, min_child_weight)
            counts["rejected"] += rejected
            if rejected:
                counts["rejected_at"][node] = rejected
            if split is None or not split[0] > oracle.RT_EPS:
                make_leaf(node, G, H)
                continue
            _, f, b, missing_left, (lg, lh) = split
            tree["state"][node], tree["feature"][node], tree["bin"][node] = oracle.SPLIT, f, b
            tree["default_left"][node] = missing_left
            wl = bounded(lg / oracle.QUANTUM, lh / oracle.QUANTUM, lam, lo, hi)[0]
            wr = bounded((G - lg) / oracle.QUANTUM, (H - lh) / oracle.QUANTUM, lam, lo, hi)[0]
            mid = (wl + wr) / 2.0
            left, right = 2 * node + 1, 2 * node + 2
            tree["lo"][left] = tree["lo"][right] = lo
            tree["hi"][left] = tree["hi"][right] = hi
            if constraints[f] > 0:
                tree["hi"][left] = tree["lo"][right] = mid
            elif constraints[f] < 0:
                tree["lo"][left] = tree["hi"][right] = mid
            x = node_bins[f, rows]
            go_left = np.where(x == oracle.MISSING, bool(missing_left), x < b)
            node_of[rows] = np.where(go_left, left, right)
            pending[left] = (lg, lh)
            pending[right] = (G - lg, H - lh)
    return tree, tree["leaf"][oracle.route(tree, node_bins)], counts


def violations(tree, constraints):
    """The splits of a heap tree on a constrained feature whose left and right leaf ranges stand in the wrong order."""
    state, slots = tree["state"], tree["state"].shape[0]
    low, high = np.zeros(slots, np.float32), np.zeros(slots, np.float32)
    count = 0
    for node in range(slots - 1, -1, -1):
        if state[node] == oracle.LEAF:
            low[node] = high[node] = tree["leaf"][node]
        elif state[node] == oracle.SPLIT:
            left, right = 2 * node + 1, 2 * node + 2
            low[node], high[node] = min(low[left], low[right]), max(high[left], high[right])
            sign = constraints[tree["feature"][node]]
            if (sign > 0 and high[left] > low[right]) or (sign < 0 and low[left] < high[right]):
                count += 1
    return count


def train(features, target, constraints, rounds, max_depth=5, eta=0.1, min_child_weight=1.0, reg_lambda=1.0, beta=5.0,
          max_bin=256):
    """Whole-oracle training under the constraints with NumPy's float32 sigmoid -> dict(trees, margins float32[n],
    rejected, clamped: totals over the run, violations: per tree)."""
    per_feature = oracle.cuts(features, max_bin)
    node_bins = oracle.bins(features, per_feature)
    counts = np.array([c.size for c in per_feature])
    leafsum = np.zeros(node_bins.shape[1], np.float32)
    out = dict(trees=[], rejected=0, clamped=0, violations=[])
    for _ in range(rounds):
        gh = oracle.gradients(oracle.sigmoid32(np.float32(0.0) + leafsum), target, beta)
        tree, leaves, seen = grow_tree(node_bins, counts, gh, constraints, max_depth, eta, min_child_weight, reg_lambda)
        leafsum = (leafsum + leaves).astype(np.float32)
        out["trees"].append(tree)
        out["rejected"] += seen["rejected"]
        out["clamped"] += seen["clamped"]
        out["violations"].append(violations(tree, constraints))
    out["margins"] = np.float32(0.0) + leafsum
    return out


def same_tree(a, b):
    """Heap trees equal in structure and in the bits of their leaves."""
    live = a["state"] != oracle.ABSENT
    return all(np.array_equal(a[key], b[key]) for key in ("state", "feature", "bin", "default_left")) and \
        np.array_equal(a["leaf"][live].view(np.uint32), b["leaf"][live].view(np.uint32))
