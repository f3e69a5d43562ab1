"""Next row f-4: the tree ensemble of predict.py:229-234 applied to the feature matrix on the GPU.

The reference pickles an `xgboost.Booster` (train.py:135, predict.py:80-82) and calls
`model.predict(xgb.DMatrix(features), ntree_limit=model.best_ntree_limit)`.  xgboost is not part of the reference tree;
a maintainer exports the booster once with `model.get_dump(dump_format='json')` (a list with one JSON string per tree)
and loads it here with `ForestModel.from_xgboost_dump(...)`.  Prediction follows xgboost's published rule for
`binary:logistic` (parity unpinned against the library itself; the GPU tests compare margins bit-for-bit with a CPU restatement of the same rule).
"""
import ctypes
import json
import math

import numpy as np

from . import _lib


def validate_cover(cover, n_nodes):
    """set_cover's checks (no library needed) -> float64[n_nodes]: one finite value above 0 per node."""
    try:
        cover = np.asarray(cover, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("cover must be an array of numbers") from None
    if cover.shape != (n_nodes,):
        raise ValueError(f"cover has shape {cover.shape}, the model has {n_nodes} nodes")
    if not np.isfinite(cover).all():
        raise ValueError(f"cover[{int(np.flatnonzero(~np.isfinite(cover))[0])}] is not finite")
    if (cover <= 0).any():
        at = int(np.flatnonzero(cover <= 0)[0])
        raise ValueError(f"cover[{at}] = {cover[at]} is not above 0")
    return np.ascontiguousarray(cover)


def cover_from_counts(counts, arrays, prior=0.0):
    """fit_cover's host step: float64[n_nodes] from the rows counted per node.  `prior` is a pseudo-count per leaf,
    added to the leaf and to every ancestor of it, so that a parent stays the sum of its two children.  Without a prior
    a node no row reached is refused by name: the contributions would divide by its cover."""
    prior = float(prior)
    if not np.isfinite(prior) or prior < 0:
        raise ValueError(f"prior must be a finite non-negative number, not {prior!r}")
    cover = np.asarray(counts).astype(np.float64)
    feature, offsets = arrays["feature"], arrays["tree_offsets"]
    if cover.shape != feature.shape:
        raise ValueError(f"{cover.shape[0]} counts for {feature.shape[0]} nodes")
    if prior > 0:
        leaves = np.zeros(feature.shape[0], dtype=np.float64)       # leaves below each node
        for t in range(offsets.shape[0] - 1):
            begin, end = int(offsets[t]), int(offsets[t + 1])
            for i in range(end - 1, begin - 1, -1):                 # children come after their parent
                if feature[i] < 0:
                    leaves[i] = 1.0
                else:
                    leaves[i] = leaves[begin + arrays["yes"][i]] + leaves[begin + arrays["no"][i]]
        cover = cover + prior * leaves
    elif (cover <= 0).any():
        at = int(np.flatnonzero(cover <= 0)[0])
        tree = int(np.searchsorted(offsets, at, side="right") - 1)
        raise ValueError(f"no row reached node {at - int(offsets[tree])} of tree {tree} (node {at} of the model): "
                         "count more rows or give a prior > 0")
    return cover


# ---- model inspection ("Model inspection"; csrc/ds_inspect.hip) ----------------------------------
INSPECT_BASELINE, INSPECT_PERMUTE, INSPECT_OVERRIDE = 0, 1, 2      # DS_INSPECT_*
INSPECT_COUNTERS = 5                                                 # tp, tn, fp, fn, margin_sum
INSPECT_JOB = np.dtype([("kind", np.int32), ("feature", np.int32), ("value", np.float32), ("repeat", np.uint32)])
INSPECT_REPEATS_MAX = 1 << 16
INSPECT_ROWS_MAX = 1 << 31
MARGIN_QUANTUM = 1 << 20                                             # margin_sum counts units of 2^-20


def _whole(name, value, low, high):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not low <= value < high:
        raise ValueError(f"{name} must be an integer in [{low}, {high}), not {value!r}")
    return int(value)


def _open_unit(name, value):
    try:
        value = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a number in (0, 1), not {value!r}") from None
    if not 0 < value < 1:           # refuses NaN too
        raise ValueError(f"{name} must be a number in (0, 1), not {value!r}")
    return value


def feature_index(feature, n_features, names=None, what="feature"):
    """A feature given as an index or, with `names`, as one of them -> its index in [0, n_features)."""
    if isinstance(feature, str):
        if names is None or feature not in names:
            raise ValueError(f"{what} {feature!r} is not one of the feature names")
        feature = list(names).index(feature)
    return _whole(what, feature, 0, n_features)


def validate_inspection(n_features, rows=None, n=None, target=None, n_repeats=1, seed=0, features=None, feature=None,
                        grid=None, n_grid=32, threshold=0.9, beta=5.0, names=None):
    """The checks of permutation_importance, partial_dependence and their device forms (no library needed) -> a dict
    of the cleaned arguments.  rows: a host [n, n_features] matrix of numbers, or None with `n` for a matrix in HBM;
    target: None or n labels of 0 / 1; features: None (all) or unique indices / names; feature: None, an index or a
    name; grid: None or a non-empty 1-D array of numbers (NaN and the infinities are values like any other)."""
    if rows is not None:
        rows = np.asarray(rows)
        if rows.ndim != 2 or rows.shape[1] != n_features:
            raise ValueError(f"rows must be a [n, {n_features}] matrix, not shape {rows.shape}")
        if not (np.issubdtype(rows.dtype, np.floating) or np.issubdtype(rows.dtype, np.integer)):
            raise ValueError(f"rows must be numbers, not {rows.dtype}")
        if n is not None and n != rows.shape[0]:
            raise ValueError(f"n = {n!r} but rows has {rows.shape[0]} rows")
        rows, n = np.ascontiguousarray(rows, dtype=np.float32), rows.shape[0]
    n = _whole("n", n, 1, INSPECT_ROWS_MAX + 1)
    if target is not None:
        target = np.asarray(target)
        if target.ndim != 1 or target.shape[0] != n:
            raise ValueError(f"target must hold {n} labels, not shape {target.shape}")
        if target.dtype == object or not np.isin(target, (0, 1)).all():
            raise ValueError("target labels must all be 0 or 1")
        target = np.ascontiguousarray(target, dtype=np.float32)
    n_repeats = _whole("n_repeats", n_repeats, 1, INSPECT_REPEATS_MAX)
    seed = _whole("seed", seed, 0, 1 << 63)
    n_grid = _whole("n_grid", n_grid, 1, INSPECT_REPEATS_MAX)
    if features is None:
        features = np.arange(n_features, dtype=np.int32)
    else:
        if isinstance(features, (str, bytes)) or not hasattr(features, "__len__"):
            raise ValueError(f"features must be a sequence of indices or names, not {features!r}")
        features = np.array([feature_index(f, n_features, names, "features") for f in features], dtype=np.int32)
        if features.shape[0] == 0:
            raise ValueError("features must not be empty")
        if np.unique(features).shape[0] != features.shape[0]:
            raise ValueError("features must be unique")
    if feature is not None:
        feature = feature_index(feature, n_features, names)
    if grid is not None:
        try:
            grid = np.asarray(grid, dtype=np.float32)
        except (TypeError, ValueError):
            raise ValueError("grid must be an array of numbers") from None
        if grid.ndim != 1 or grid.shape[0] == 0:
            raise ValueError(f"grid must be 1-D and non-empty, not shape {grid.shape}")
        grid = np.ascontiguousarray(grid)
    threshold = _open_unit("threshold", threshold)
    try:
        beta = float(beta)
    except (TypeError, ValueError):
        raise ValueError(f"beta must be a positive number, not {beta!r}") from None
    if not (np.isfinite(beta) and beta > 0):
        raise ValueError(f"beta must be a finite positive number, not {beta!r}")
    return dict(rows=rows, n=n, target=target, n_repeats=n_repeats, seed=seed, features=features, feature=feature,
                grid=grid, n_grid=n_grid, threshold=threshold, beta=beta)


def inspection_jobs(jobs):
    """(kind, feature, value, repeat) tuples -> the job table of ds_forest_inspect (INSPECT_JOB records)."""
    table = np.zeros(len(jobs), dtype=INSPECT_JOB)
    for at, (kind, feature, value, repeat) in enumerate(jobs):
        table[at] = (kind, feature, value, repeat)
    return table


def permutation_jobs(features, n_repeats):
    """One baseline job, then for every feature of `features` its n_repeats permute jobs."""
    table = np.zeros(1 + len(features) * n_repeats, dtype=INSPECT_JOB)
    table["kind"][1:] = INSPECT_PERMUTE
    table["feature"][1:] = np.repeat(np.asarray(features, dtype=np.int32), n_repeats)
    table["repeat"][1:] = np.tile(np.arange(n_repeats, dtype=np.uint32), len(features))
    return table


def dependence_jobs(feature, grid):
    """One baseline job, then one override job per grid value."""
    table = np.zeros(1 + grid.shape[0], dtype=INSPECT_JOB)
    table["kind"][1:] = INSPECT_OVERRIDE
    table["feature"][1:] = feature
    table["value"][1:] = grid
    return table


def quantile_grid(column, n_grid):
    """partial_dependence's default grid, float32: the distinct values among the n_grid evenly spaced order statistics
    v[(k * (m - 1)) // max(n_grid - 1, 1)], k = 0 .. n_grid - 1, of the column's m sorted non-NaN values, ascending, and
    one NaN last when the column has any."""
    column = np.asarray(column, dtype=np.float32)
    missing = np.isnan(column)
    values = np.sort(column[~missing])
    grid = np.zeros(0, np.float32)
    if values.shape[0]:
        at = (np.arange(n_grid, dtype=np.int64) * (values.shape[0] - 1)) // max(n_grid - 1, 1)
        grid = np.unique(values[at])
    if missing.any():
        grid = np.concatenate([grid, np.array([np.nan], np.float32)])
    return grid.astype(np.float32)


def _margin_sums(counters):
    return counters[:, 4].astype(np.uint64).view(np.int64)


class PermutationImportance:
    """What ForestModel.permutation_importance returns, derived on the host in float64 from the integers of one launch
    (`counters`: uint64[1 + n_selected * n_repeats, 5], the baseline job first):
    baseline (tp, tn, fp, fn) and baseline_error = fn + beta * fp of the unchanged matrix; error_matrix
    int64[n_selected, n_repeats, 4] and errors float64[n_selected, n_repeats] with feature features[s] shuffled;
    importance = the mean over the repeats of errors - baseline_error, importance_std its population standard
    deviation; margin_shift = the mean over the repeats of the change of the mean margin."""

    def __init__(self, counters, n, features, n_repeats, seed, threshold=0.9, beta=5.0):
        counters = np.asarray(counters, dtype=np.uint64)
        self.counters, self.n = counters, int(n)
        self.features, self.n_repeats, self.seed = np.asarray(features, dtype=np.int32), int(n_repeats), int(seed)
        self.threshold, self.beta = float(threshold), float(beta)
        selected = self.features.shape[0]
        self.baseline = tuple(int(v) for v in counters[0, :4])
        self.baseline_error = self.baseline[3] + self.beta * self.baseline[2]
        self.error_matrix = counters[1:, :4].astype(np.int64).reshape(selected, self.n_repeats, 4)
        self.errors = self.error_matrix[:, :, 3].astype(np.float64) + \
            self.beta * self.error_matrix[:, :, 2].astype(np.float64)
        increase = self.errors - self.baseline_error
        self.importance = increase.mean(axis=1)
        self.importance_std = increase.std(axis=1)
        sums = _margin_sums(counters)
        shift = (sums[1:] - sums[0]).astype(np.float64).reshape(selected, self.n_repeats) / MARGIN_QUANTUM / self.n
        self.baseline_mean_margin = float(sums[0]) / MARGIN_QUANTUM / self.n
        self.margin_shift = shift.mean(axis=1)

    def order(self):
        """The positions of `features` by importance, descending, ties to the lower feature."""
        return np.lexsort((self.features, -self.importance))

    def frame(self, names=None):
        """A DataFrame (feature, name, importance, importance_std, margin_shift) sorted by importance, descending, ties
        to the lower feature.  names: FEATURE_NAMES by default; a feature beyond them is called f<index>."""
        import pandas as pd
        if names is None:
            from .feature_engineering import FEATURE_NAMES as names
        order = self.order()
        features = self.features[order]
        return pd.DataFrame({"feature": features,
                             "name": [names[f] if f < len(names) else f"f{f}" for f in features],
                             "importance": self.importance[order], "importance_std": self.importance_std[order],
                             "margin_shift": self.margin_shift[order]})


class PartialDependence:
    """What ForestModel.partial_dependence returns (`counters`: uint64[1 + len(grid), 5], the baseline job first):
    `grid` float32; mean_margin float64[len(grid)] = margin_sum / 2^20 / n with the feature set to the grid value in
    every row; positive_share = the share of rows above the threshold then; baseline_mean_margin of the unchanged
    matrix; error_matrix int64[len(grid), 4] (with a target; all rows count as label 0 without one)."""

    def __init__(self, counters, n, feature, grid, threshold=0.9):
        counters = np.asarray(counters, dtype=np.uint64)
        self.counters, self.n, self.feature = counters, int(n), int(feature)
        self.grid, self.threshold = np.asarray(grid, dtype=np.float32), float(threshold)
        sums = _margin_sums(counters)
        self.baseline_mean_margin = float(sums[0]) / MARGIN_QUANTUM / self.n
        self.mean_margin = sums[1:].astype(np.float64) / MARGIN_QUANTUM / self.n
        self.error_matrix = counters[1:, :4].astype(np.int64)
        self.positive_share = (self.error_matrix[:, 0] + self.error_matrix[:, 2]).astype(np.float64) / self.n


# ---- refreshing a model ("Refreshing a model"; csrc/ds_refresh.hip) ------------------------------
GRADIENT_QUANTUM = float(1 << 30)                                    # node_sums count units of 2^-30


def validate_refresh(n_features, features=None, target=None, eval_features=None, eval_target=None, *, n=None,
                     n_eval=0, eta=0.1, reg_lambda=1.0, beta=5.0, sample_weight=None, refresh_leaf=True):
    """The checks of ForestModel.refresh and refresh_device (no library needed) -> a dict of the cleaned arguments.
    features: a host [n, n_features] matrix of numbers, n >= 0 (no row: the model comes back unchanged), or None with
    `n` for a matrix in HBM; target: n labels of 0 / 1.  eval_features / eval_target go together: a host
    [n_eval, n_features] matrix with n_eval >= 1, or, for a matrix in HBM, eval_target with n_eval given.  eta and beta
    finite and above 0, reg_lambda finite and not negative; sample_weight: None or train.validate_sample_weight's;
    without weights max(beta, 1) * n <= 2^32, the same bound on the integer sums; refresh_leaf a bool."""
    from .train import WEIGHT_GUARD, _labels, _real, validate_sample_weight

    def matrix(rows, rows_n, what, low):
        if rows is None:
            if isinstance(rows_n, bool) or not isinstance(rows_n, (int, np.integer)) or not low <= rows_n < 1 << 31:
                raise ValueError(f"the number of {what} rows must be an integer in [{low}, 2^31), not {rows_n!r}")
            return None, int(rows_n)
        rows = np.asarray(rows)
        if rows.ndim != 2 or rows.shape[1] != n_features:
            raise ValueError(f"{what} features must be a [n, {n_features}] matrix, not shape {rows.shape}")
        if not (np.issubdtype(rows.dtype, np.floating) or np.issubdtype(rows.dtype, np.integer)):
            raise ValueError(f"{what} features must be numbers, not {rows.dtype}")
        if rows.shape[0] < low:
            raise ValueError(f"{what} features need at least {low} row")
        return np.ascontiguousarray(rows, dtype=np.float32), rows.shape[0]

    features, n = matrix(features, n, "training", 0)
    if target is None:
        raise ValueError("target is missing: a refresh needs one label per training row")
    target = _labels(n, target, "training")
    has_eval = eval_target is not None
    if features is not None and (eval_features is None) != (eval_target is None):
        raise ValueError("eval_features and eval_target go together")
    if has_eval:
        eval_features, n_eval = matrix(eval_features, n_eval, "evaluation", 1)
        eval_target = _labels(n_eval, eval_target, "evaluation")
    else:
        eval_features, n_eval = None, 0
    eta, reg_lambda = _real("eta", eta, positive=True), _real("reg_lambda", reg_lambda)
    beta = _real("beta", beta, positive=True)
    if sample_weight is not None:
        sample_weight = validate_sample_weight(sample_weight, n, beta)
    elif max(beta, 1.0) * n > WEIGHT_GUARD:
        raise ValueError(f"max(beta, 1) * n = {max(beta, 1.0) * n!r} exceeds 2^32: the integer sums could overflow")
    if not isinstance(refresh_leaf, (bool, np.bool_)):
        raise ValueError(f"refresh_leaf must be True or False, not {refresh_leaf!r}")
    return dict(features=features, n=n, target=target, eval_features=eval_features, n_eval=n_eval,
                eval_target=eval_target, eta=eta, reg_lambda=reg_lambda, beta=beta, sample_weight=sample_weight,
                refresh_leaf=bool(refresh_leaf))


def split_gains(arrays, node_sums, reg_lambda):
    """float64[n_nodes]: for every split node G_L^2 / (H_L + lambda) + G_R^2 / (H_R + lambda) - G^2 / (H + lambda) of
    its own and its two children's (G, H) = node_sums / 2^30, the trainer's split gain on the refreshed data; 0 for a
    leaf.  No library needed."""
    sums = np.asarray(node_sums, dtype=np.int64).astype(np.float64) / GRADIENT_QUANTUM
    feature, offsets = arrays["feature"], arrays["tree_offsets"]
    tree = np.searchsorted(offsets, np.arange(feature.shape[0]), side="right") - 1
    base = offsets[tree] if feature.shape[0] else np.zeros(0, np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        term = sums[:, 0] * sums[:, 0] / (sums[:, 1] + float(reg_lambda))
    term = np.where(np.isfinite(term), term, 0.0)             # lambda = 0 and no hessian: no evidence, no gain
    split = feature >= 0
    gain = np.zeros(feature.shape[0], np.float64)
    gain[split] = term[(base + arrays["yes"])[split]] + term[(base + arrays["no"])[split]] - term[split]
    return gain


class RefreshResult:
    """What ForestModel.refresh returns.  `model`: a NEW ForestModel with the old model's splits and base margin and
    the refreshed leaves (refresh_leaf=False: the old leaves); node_sums int64[n_nodes, 2]: the (gradient, hessian) sums
    in units of 2^-30 of the rows that reach each node; cover float64[n_nodes] = hessian sum / 2^30 (xgboost's cover);
    gain float64[n_nodes]: split_gains, 0 for a leaf; empty_leaves: the leaves whose hessian sum is 0, which kept their
    value; margins float32[n]: the refreshed model's margins of the training rows.  With an evaluation set: history, the
    custom error after every tree prefix of the refreshed model (n_trees values), best_iteration, the prefix (from 0)
    of its first minimum, and initial_error, the error of the model as given; None otherwise."""

    def __init__(self, model, node_sums, empty_leaves, margins, reg_lambda, eval_errors=None):
        self.model, self.node_sums, self.empty_leaves, self.margins = model, node_sums, int(empty_leaves), margins
        self.reg_lambda = float(reg_lambda)
        self.cover = node_sums[:, 1].astype(np.float64) / GRADIENT_QUANTUM
        self.gain = split_gains(model.arrays, node_sums, reg_lambda)
        self.history = self.initial_error = self.best_iteration = None
        if eval_errors is not None:
            from .train import FirstMinimum
            self.initial_error, self.history = int(eval_errors[0]), [int(v) for v in eval_errors[1:]]
            rule = FirstMinimum()
            for round_, value in enumerate(self.history):
                rule.see(round_, value)
            self.best_iteration = rule.best

    def gain_importance(self):
        """float64[n_features]: per feature the total gain of its splits over the sum of them, the shape of
        ForestModel.feature_importance(); zeros when no split gains anything.  A split whose gain on this data is
        negative counts as it is."""
        feature = self.model.arrays["feature"]
        split = feature >= 0
        totals = np.bincount(feature[split], weights=self.gain[split], minlength=self.model.n_features)
        total = totals.sum()
        return totals / total if total else np.zeros(self.model.n_features, np.float64)


class ForestModel:
    def __init__(self, feature, threshold, yes, no, missing, tree_offsets, n_features, base_margin=0.0, device=0):
        self.arrays = dict(feature=np.ascontiguousarray(feature, dtype=np.int32),
                           threshold=np.ascontiguousarray(threshold, dtype=np.float32),
                           yes=np.ascontiguousarray(yes, dtype=np.int32), no=np.ascontiguousarray(no, dtype=np.int32),
                           missing=np.ascontiguousarray(missing, dtype=np.int32),
                           tree_offsets=np.ascontiguousarray(tree_offsets, dtype=np.int64),
                           base_margin=float(base_margin))
        self.n_features = int(n_features)
        self.n_trees = self.arrays["tree_offsets"].shape[0] - 1
        self.device = device
        self.cover = None
        self.handle = ctypes.c_void_p()
        a = self.arrays
        _lib.check(_lib.lib().ds_forest_create(_lib.pointer(a["feature"]), _lib.pointer(a["threshold"]), _lib.pointer(a["yes"]), _lib.pointer(a["no"]),
                                               _lib.pointer(a["missing"]), _lib.pointer(a["tree_offsets"]), self.n_trees,
                                               self.n_features, ctypes.c_float(a["base_margin"]), device,
                                               ctypes.byref(self.handle)), "ds_forest_create")

    @staticmethod
    def parse_xgboost_dump(trees, ntree_limit=None, base_score=0.5):
        """`Booster.get_dump(dump_format='json')` -> the flat arrays (feature names 'f<index>')."""
        if ntree_limit:
            trees = trees[:ntree_limit]                       # predict.py:232 ntree_limit=best_ntree_limit
        feature, threshold, yes, no, missing, offsets = [], [], [], [], [], [0]
        for text in trees:
            root = json.loads(text) if isinstance(text, str) else text
            nodes = {}
            stack = [root]
            while stack:
                node = stack.pop()
                nodes[int(node["nodeid"])] = node
                stack.extend(node.get("children", ()))
            size = max(nodes) + 1
            f = np.full(size, -1, np.int32)
            t = np.zeros(size, np.float32)
            y = np.zeros(size, np.int32)
            n = np.zeros(size, np.int32)
            m = np.zeros(size, np.int32)
            for nodeid, node in nodes.items():
                if "leaf" in node:
                    t[nodeid] = np.float32(node["leaf"])
                else:
                    split = node["split"]
                    f[nodeid] = int(split[1:]) if isinstance(split, str) else int(split)
                    t[nodeid] = np.float32(node["split_condition"])
                    y[nodeid], n[nodeid], m[nodeid] = int(node["yes"]), int(node["no"]), int(node["missing"])
            feature.append(f); threshold.append(t); yes.append(y); no.append(n); missing.append(m)
            offsets.append(offsets[-1] + size)
        cat = lambda parts, dtype: np.concatenate(parts).astype(dtype) if parts else np.zeros(0, dtype)
        base_margin = math.log(base_score / (1.0 - base_score))
        return dict(feature=cat(feature, np.int32), threshold=cat(threshold, np.float32), yes=cat(yes, np.int32),
                    no=cat(no, np.int32), missing=cat(missing, np.int32),
                    tree_offsets=np.array(offsets, dtype=np.int64), base_margin=base_margin)

    @staticmethod
    def parse_xgboost_model_json(model, ntree_limit=None):
        """`Booster.save_model('model.json')` (xgboost >= 1.0) -> the flat arrays.  Unlike the text dump, this format
        carries every split condition and leaf value as the exact float32 the booster holds."""
        if isinstance(model, (str, bytes)):
            model = json.loads(model)
        learner = model["learner"]
        trees = learner["gradient_booster"]["model"]["trees"]
        if ntree_limit:
            trees = trees[:ntree_limit]
        feature, threshold, yes, no, missing, offsets = [], [], [], [], [], [0]
        for tree in trees:
            left = np.asarray(tree["left_children"], dtype=np.int32)
            right = np.asarray(tree["right_children"], dtype=np.int32)
            leaf = left < 0
            f = np.where(leaf, -1, np.asarray(tree["split_indices"], dtype=np.int32)).astype(np.int32)
            t = np.asarray(tree["split_conditions"], dtype=np.float32)      # leaves: the leaf value
            default_left = np.asarray(tree["default_left"], dtype=bool)
            feature.append(f); threshold.append(t)
            yes.append(np.where(leaf, 0, left)); no.append(np.where(leaf, 0, right))
            missing.append(np.where(leaf, 0, np.where(default_left, left, right)))
            offsets.append(offsets[-1] + left.shape[0])
        cat = lambda parts, dtype: np.concatenate(parts).astype(dtype) if parts else np.zeros(0, dtype)
        base_score = float(learner["learner_model_param"]["base_score"])
        return dict(feature=cat(feature, np.int32), threshold=cat(threshold, np.float32), yes=cat(yes, np.int32),
                    no=cat(no, np.int32), missing=cat(missing, np.int32),
                    tree_offsets=np.array(offsets, dtype=np.int64),
                    base_margin=math.log(base_score / (1.0 - base_score)))

    @classmethod
    def from_xgboost_model_json(cls, model, n_features, ntree_limit=None, device=0):
        a = cls.parse_xgboost_model_json(model, ntree_limit)
        return cls(a["feature"], a["threshold"], a["yes"], a["no"], a["missing"], a["tree_offsets"], n_features,
                   a["base_margin"], device)

    @classmethod
    def from_xgboost_dump(cls, trees, n_features, ntree_limit=None, base_score=0.5, device=0):
        a = cls.parse_xgboost_dump(trees, ntree_limit, base_score)
        return cls(a["feature"], a["threshold"], a["yes"], a["no"], a["missing"], a["tree_offsets"], n_features,
                   a["base_margin"], device)

    @classmethod
    def from_trees(cls, trees, n_features, base_margin=0.0, device=0):
        """One model from per-tree dicts of feature / threshold / yes / no / missing arrays (tree-relative ids)."""
        offsets = np.zeros(len(trees) + 1, np.int64)
        offsets[1:] = np.cumsum([tree["feature"].shape[0] for tree in trees])
        cat = lambda key, dtype: np.concatenate([tree[key] for tree in trees]).astype(dtype) if trees else np.zeros(0, dtype)
        return cls(cat("feature", np.int32), cat("threshold", np.float32), cat("yes", np.int32), cat("no", np.int32),
                   cat("missing", np.int32), offsets, n_features, base_margin, device)

    TREE_KEYS = ("feature", "threshold", "yes", "no", "missing")

    @staticmethod
    def head_arrays(arrays, n_trees):
        """The flat arrays of the first n_trees trees of `arrays` (no library needed)."""
        total = arrays["tree_offsets"].shape[0] - 1
        if isinstance(n_trees, bool) or not isinstance(n_trees, (int, np.integer)) or not 0 <= n_trees <= total:
            raise ValueError(f"n_trees must be an integer in [0, {total}], not {n_trees!r}")
        end = int(arrays["tree_offsets"][n_trees])
        out = {key: arrays[key][:end].copy() for key in ForestModel.TREE_KEYS}
        return dict(out, tree_offsets=arrays["tree_offsets"][:int(n_trees) + 1].copy(), base_margin=arrays["base_margin"])

    @staticmethod
    def extended_arrays(arrays, trees):
        """The flat arrays of `arrays`' trees followed by `trees`, per-tree dicts as from_trees takes them (no library
        needed)."""
        trees = list(trees)
        dtypes = dict(feature=np.int32, threshold=np.float32, yes=np.int32, no=np.int32, missing=np.int32)
        sizes = [np.asarray(tree["feature"]).shape[0] for tree in trees]
        out = {key: np.concatenate([arrays[key]] + [np.asarray(tree[key], dtype=dtypes[key]) for tree in trees])
               for key in ForestModel.TREE_KEYS}
        offsets = np.concatenate([arrays["tree_offsets"],
                                  arrays["tree_offsets"][-1] + np.cumsum(sizes, dtype=np.int64)]).astype(np.int64)
        return dict(out, tree_offsets=offsets, base_margin=arrays["base_margin"])

    @staticmethod
    def tree_list(arrays):
        """The per-tree dicts (views) of flat arrays: what from_trees and extended take."""
        offsets = arrays["tree_offsets"]
        return [{key: arrays[key][int(offsets[t]):int(offsets[t + 1])] for key in ForestModel.TREE_KEYS}
                for t in range(offsets.shape[0] - 1)]

    @staticmethod
    def monotone_violations_of(arrays, constraints):
        """monotone_violations of flat arrays (no library needed); `constraints`: one sign per feature index."""
        feature, value, yes, no = arrays["feature"], arrays["threshold"], arrays["yes"], arrays["no"]
        offsets = arrays["tree_offsets"]
        violations = 0
        for t in range(offsets.shape[0] - 1):
            begin, size = int(offsets[t]), int(offsets[t + 1] - offsets[t])
            if size == 0:
                continue
            order, at = [0], 0                                   # parents before their children, whatever the ids
            while at < len(order):
                i = order[at]
                at += 1
                if feature[begin + i] >= 0:
                    order += [int(yes[begin + i]), int(no[begin + i])]
            low, high = np.zeros(size, np.float32), np.zeros(size, np.float32)     # the leaf range below each node
            for i in reversed(order):
                f = int(feature[begin + i])
                if f < 0:
                    low[i] = high[i] = value[begin + i]
                    continue
                left, right = int(yes[begin + i]), int(no[begin + i])            # x < threshold, x >= threshold
                low[i], high[i] = min(low[left], low[right]), max(high[left], high[right])
                sign = int(constraints[f]) if f < len(constraints) else 0
                if (sign > 0 and high[left] > low[right]) or (sign < 0 and low[left] < high[right]):
                    violations += 1
        return violations

    def monotone_violations(self, constraints):
        """The number of splits on a constrained feature whose subtrees stand in the wrong order: for a sign of +1 the
        largest leaf below the `yes` child (x < threshold) exceeds the smallest below the `no` child, for -1 the
        reverse.  0 means every tree, and so the margin, is monotone in each constrained feature; a row with the
        feature missing follows the split's default branch and is outside the claim.  A host function of the arrays
        alone, so it judges xgboost imports too.  constraints: train.validate_monotone_constraints' sequence form."""
        from .train import validate_monotone_constraints
        return self.monotone_violations_of(self.arrays, validate_monotone_constraints(constraints, self.n_features))

    def _from_arrays(self, a):
        return type(self)(a["feature"], a["threshold"], a["yes"], a["no"], a["missing"], a["tree_offsets"],
                          self.n_features, a["base_margin"], self.device)

    def head(self, n_trees):
        """A new model of the first n_trees trees (0 .. self.n_trees; 0: the empty forest, whose margin is the base
        margin), without a cover."""
        return self._from_arrays(self.head_arrays(self.arrays, n_trees))

    def extended(self, trees):
        """A new model of this model's trees followed by `trees`, per-tree dicts as from_trees takes them (those of
        another model: tree_list(other.arrays)).  The result has this model's base margin and NO cover: a cover
        describes the forest it was counted for."""
        return self._from_arrays(self.extended_arrays(self.arrays, trees))

    def save(self, path):
        """The flat arrays in one .npz (the reference pickles its booster, train.py:134-135)."""
        a = self.arrays
        extra = {} if self.cover is None else {"cover": self.cover}     # a model without cover: the file of before
        with open(path, "wb") as handle:
            np.savez(handle, feature=a["feature"], threshold=a["threshold"], yes=a["yes"], no=a["no"],
                     missing=a["missing"], tree_offsets=a["tree_offsets"],
                     base_margin=np.float64(a["base_margin"]), n_features=np.int64(self.n_features), **extra)

    @classmethod
    def load(cls, path, device=0):
        with np.load(path, allow_pickle=False) as saved:
            a = {key: saved[key] for key in saved.files}
        model = cls(a["feature"], a["threshold"], a["yes"], a["no"], a["missing"], a["tree_offsets"],
                    int(a["n_features"]), float(a["base_margin"]), device)
        if "cover" in a:
            model.set_cover(a["cover"])
        return model

    @staticmethod
    def xgboost_cover(model_json, ntree_limit=None):
        """float64[n_nodes]: the `sum_hessian` of every node of a `Booster.save_model('model.json')`, in the node order
        of parse_xgboost_model_json, for set_cover (what xgboost's own pred_contribs weighs with)."""
        if isinstance(model_json, (str, bytes)):
            model_json = json.loads(model_json)
        trees = model_json["learner"]["gradient_booster"]["model"]["trees"]
        if ntree_limit:
            trees = trees[:ntree_limit]
        parts = [np.asarray(tree["sum_hessian"], dtype=np.float64) for tree in trees]
        return np.concatenate(parts) if parts else np.zeros(0, np.float64)

    @property
    def n_nodes(self):
        return int(self.arrays["feature"].shape[0])

    def set_cover(self, cover):
        """Install the node cover (float64[n_nodes], every entry finite and above 0; None removes it): the weight of
        the background rows that reach each node, which predict_contributions weighs the branches with."""
        if cover is None:
            _lib.check(_lib.lib().ds_forest_cover_clear(self.handle), "ds_forest_cover_clear")
            self.cover = None
            return
        cover = validate_cover(cover, self.n_nodes)
        _lib.check(_lib.lib().ds_forest_cover_set(self.handle, _lib.pointer(cover)), "ds_forest_cover_set")
        self.cover = cover

    def fit_cover(self, rows, prior=0.0):
        """The cover counted from a host float32[n, n_features] matrix (see fit_cover_device)."""
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        if rows.ndim != 2 or rows.shape[1] != self.n_features:
            raise ValueError(f"rows must be a [n, {self.n_features}] matrix, not shape {rows.shape}")
        cover_from_counts(np.ones(self.n_nodes), self.arrays, prior)        # prior's own check, before any device work
        d_rows = _lib.DeviceArray.from_host(rows if rows.shape[0] else np.zeros((1, self.n_features), np.float32),
                                            self.device)
        try:
            return self.fit_cover_device(d_rows, rows.shape[0], prior)
        finally:
            d_rows.free()

    def fit_cover_device(self, d_rows, n, prior=0.0):
        """Count the first n rows of a float32[n, n_features] matrix in HBM through every tree on the device
        (ds_forest_cover_device: exact integer counts per node) and install the result as the cover.  prior: a
        pseudo-count per leaf, added on the host to the leaf and all of its ancestors.  Without one, a node no row
        reached is a ValueError that names it (the model then keeps the cover it had).  Returns the cover."""
        cover_from_counts(np.ones(self.n_nodes), self.arrays, prior)
        counts = self.count_cover_device(d_rows, n)
        previous = self.cover
        try:
            cover = cover_from_counts(counts, self.arrays, prior)
        except ValueError:
            self.set_cover(previous)
            raise
        self.set_cover(cover)
        return cover

    def count_cover_device(self, d_rows, n, accumulate=False, stream=None):
        """float64[n_nodes]: the rows of the matrix in HBM that reach each node, counted on the device into the
        forest's counters (from zero, or on top of the last count when `accumulate`).  The counters stay the forest's
        cover until set_cover replaces them."""
        library = _lib.lib()
        if not accumulate:
            _lib.check(library.ds_forest_cover_clear(self.handle), "ds_forest_cover_clear")
        _lib.check(library.ds_forest_cover_device(self.handle, _lib.pointer(d_rows), int(n), _lib.pointer(stream)),
                   "ds_forest_cover_device")
        self.cover = None
        return self.read_cover()

    def read_cover(self):
        """float64[n_nodes] as the library holds it (ds_forest_cover_read): the installed cover, or the counters."""
        out = np.empty(self.n_nodes, dtype=np.float64)
        _lib.check(_lib.lib().ds_forest_cover_read(self.handle, _lib.pointer(out)), "ds_forest_cover_read")
        return out

    def option(self, name, value):
        """ds_forest_option, for tests: option("max_blocks", v) caps the grids of the cover, contributions and inspection
        kernels and of refresh's row kernels; option("inspect_jobs_per_block", v) sets the jobs an inspection workgroup
        runs per staged row block; option("refresh_lds_nodes", v) the largest tree (in nodes, at most 2048) whose sums a
        refresh workgroup keeps in LDS, a larger tree adding straight to HBM."""
        _lib.set_option("ds_forest_option", name, value, self.handle)

    def predict_contributions(self, rows, approximate=False):
        """float64[n, n_features + 1] for a host float32[n, n_features] matrix: per row the contribution of every
        feature to the margin and, last, the bias (xgboost's predict(pred_contribs=True): path-dependent TreeSHAP;
        approximate=True: approx_contribs, Saabas).  Needs a cover (set_cover / fit_cover)."""
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        assert rows.ndim == 2 and rows.shape[1] == self.n_features
        out = np.empty((rows.shape[0], self.n_features + 1), dtype=np.float64)
        _lib.check(_lib.lib().ds_forest_contributions(self.handle, _lib.pointer(rows), rows.shape[0],
                                                      _lib.pointer(out), int(bool(approximate))),
                   "ds_forest_contributions")
        return out

    def predict_contributions_device(self, d_rows, n, d_out, approximate=False, stream=None):
        """predict_contributions for n rows in HBM into d_out (float64[n, n_features + 1] in HBM), enqueued on
        `stream`."""
        _lib.check(_lib.lib().ds_forest_contributions_device(self.handle, _lib.pointer(d_rows), int(n),
                                                             _lib.pointer(d_out), int(bool(approximate)),
                                                             _lib.pointer(stream)), "ds_forest_contributions_device")

    def inspect(self, rows, target, jobs, seed=0, threshold=0.9):
        """uint64[n_jobs, 5] (tp, tn, fp, fn, margin_sum in two's complement) of a job table (INSPECT_JOB records,
        inspection_jobs) over a host float32[n, n_features] matrix: ds_forest_inspect, one launch.  target: float32[n]
        or None (every label 0)."""
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        assert rows.ndim == 2 and rows.shape[1] == self.n_features
        jobs = np.ascontiguousarray(jobs, dtype=INSPECT_JOB)
        if target is not None:
            target = np.ascontiguousarray(target, dtype=np.float32)
            assert target.shape == (rows.shape[0],)
        out = np.zeros((jobs.shape[0], INSPECT_COUNTERS), dtype=np.uint64)
        _lib.check(_lib.lib().ds_forest_inspect(self.handle, _lib.pointer(rows), rows.shape[0], _lib.pointer(target),
                                                _lib.pointer(jobs), jobs.shape[0], int(seed), float(threshold),
                                                _lib.pointer(out)), "ds_forest_inspect")
        return out

    def inspect_device(self, d_rows, n, d_target, jobs, seed=0, threshold=0.9, stream=None):
        """inspect for the first n rows of a float32 matrix in HBM and a float32[n] target in HBM (or None): the job
        table is uploaded, the counters come back behind a synchronisation of `stream`."""
        jobs = np.ascontiguousarray(jobs, dtype=INSPECT_JOB)
        out = np.zeros((jobs.shape[0], INSPECT_COUNTERS), dtype=np.uint64)
        if jobs.shape[0] == 0:
            return out
        d_jobs = _lib.DeviceArray.from_host(jobs.view(np.uint8), self.device)
        d_out = _lib.DeviceArray(out.shape, np.uint64, self.device)
        try:
            _lib.check(_lib.lib().ds_forest_inspect_device(self.handle, _lib.pointer(d_rows), int(n),
                                                           _lib.pointer(d_target), d_jobs.ptr, jobs.shape[0], int(seed),
                                                           float(threshold), d_out.ptr, _lib.pointer(stream)),
                       "ds_forest_inspect_device")
            _lib.check(_lib.lib().ds_stream_sync(_lib.pointer(stream), self.device), "ds_stream_sync")
            return d_out.to_host()
        finally:
            d_jobs.free()
            d_out.free()

    def permutation_importance(self, rows, target, n_repeats=5, seed=0, features=None, threshold=0.9, beta=5.0):
        """How much the evaluation error fn + beta * fp at `threshold` grows when a feature's column is shuffled among
        the rows (a closed-form permutation of (seed, feature, repeat, n): DESIGN.md section 8, "Model inspection"),
        for every feature of `features` (indices or FEATURE_NAMES; None: all) and n_repeats shuffles each ->
        PermutationImportance.  One launch of 1 + n_selected * n_repeats jobs over the matrix, uploaded once; integer
        counts, so the same result run after run.  validate_inspection says what is accepted."""
        from .feature_engineering import FEATURE_NAMES
        v = validate_inspection(self.n_features, rows=rows, target=target, n_repeats=n_repeats, seed=seed,
                                features=features, threshold=threshold, beta=beta, names=FEATURE_NAMES)
        counters = self.inspect(v["rows"], v["target"], permutation_jobs(v["features"], v["n_repeats"]), v["seed"],
                                v["threshold"])
        return PermutationImportance(counters, v["n"], v["features"], v["n_repeats"], v["seed"], v["threshold"],
                                     v["beta"])

    def permutation_importance_device(self, d_rows, n, d_target, n_repeats=5, seed=0, features=None, threshold=0.9,
                                      beta=5.0, stream=None):
        """permutation_importance for the first n rows of a matrix that lies in HBM (train_model's evaluation matrix,
        DeviceDataSets) with its float32[n] target in HBM, or None for no labels."""
        from .feature_engineering import FEATURE_NAMES
        v = validate_inspection(self.n_features, n=n, n_repeats=n_repeats, seed=seed, features=features,
                                threshold=threshold, beta=beta, names=FEATURE_NAMES)
        counters = self.inspect_device(d_rows, v["n"], d_target, permutation_jobs(v["features"], v["n_repeats"]),
                                       v["seed"], v["threshold"], stream)
        return PermutationImportance(counters, v["n"], v["features"], v["n_repeats"], v["seed"], v["threshold"],
                                     v["beta"])

    def partial_dependence(self, rows, feature, grid=None, n_grid=32, target=None, threshold=0.9):
        """The mean margin of the rows with `feature` (an index or one of FEATURE_NAMES) set to each value of `grid` in
        every row -> PartialDependence.  grid=None: quantile_grid(rows[:, feature], n_grid), taken on the host.  One
        launch of 1 + len(grid) jobs."""
        from .feature_engineering import FEATURE_NAMES
        v = validate_inspection(self.n_features, rows=rows, target=target, feature=0 if feature is None else feature,
                                grid=grid, n_grid=n_grid, threshold=threshold, names=FEATURE_NAMES)
        if feature is None:
            raise ValueError("feature must be an index or a name, not None")
        grid = quantile_grid(v["rows"][:, v["feature"]], v["n_grid"]) if v["grid"] is None else v["grid"]
        counters = self.inspect(v["rows"], v["target"], dependence_jobs(v["feature"], grid), 0, v["threshold"])
        return PartialDependence(counters, v["n"], v["feature"], grid, v["threshold"])

    def partial_dependence_device(self, d_rows, n, feature, grid, d_target=None, threshold=0.9, stream=None):
        """partial_dependence for the first n rows of a matrix in HBM; the grid must be given."""
        from .feature_engineering import FEATURE_NAMES
        if grid is None or feature is None:
            raise ValueError("grid and feature must be given for a matrix in HBM")
        v = validate_inspection(self.n_features, n=n, feature=feature, grid=grid, threshold=threshold,
                                names=FEATURE_NAMES)
        counters = self.inspect_device(d_rows, v["n"], d_target, dependence_jobs(v["feature"], v["grid"]), 0,
                                       v["threshold"], stream)
        return PartialDependence(counters, v["n"], v["feature"], v["grid"], v["threshold"])

    def refresh(self, features, target, eval_features=None, eval_target=None, *, eta=0.1, reg_lambda=1.0, beta=5.0,
                sample_weight=None, refresh_leaf=True, trace=False):
        """Re-estimate this model's leaves on rows it may never have seen and keep every split (xgboost's
        process_type="update", updater="refresh", refresh_leaf; DESIGN.md section 9, "Refreshing a model") ->
        RefreshResult.  The rows go through the trees in order on the device: before tree t a row's gradient pair is
        taken at its margin under the trees refreshed so far (the trainer's weighted log loss, its 2^30 fixed point and
        its sample_weight), the pairs are summed per leaf as exact integers, and a leaf with a hessian sum above 0 takes
        -G / (H + reg_lambda) * eta, the trainer's leaf value; a leaf without evidence (no row, or only rows of weight
        0) keeps its value and is counted in empty_leaves.  A model grown by ForestTrainer without subsampling or
        constraints and refreshed on its own data and parameters comes back bit for bit.  This model is untouched: the
        result's `model` is a new one, without a cover (the result's `cover` can be installed with set_cover where every
        node has some).  refresh_leaf=False changes no leaf and still returns the sums, cover, gain and errors.
        eval_features / eval_target: the custom error of the refreshed model after every tree prefix (`history`,
        `best_iteration`) and that of this model (`initial_error`).  validate_refresh says what is accepted.
        Not done here: subsampling; reapplying monotone bounds (monotone_violations tells afterwards whether the
        refreshed model still satisfies them); batched or cross-validated refresh; changing any split.
        trace=True (for tests) also returns, as the result's `trace`, float32[n_trees, n]: the probabilities the
        gradients of every tree were taken at."""
        v = validate_refresh(self.n_features, features, target, eval_features, eval_target, eta=eta,
                             reg_lambda=reg_lambda, beta=beta, sample_weight=sample_weight, refresh_leaf=refresh_leaf)
        return self._refresh(False, v["features"], v["eval_features"], v, trace, None)

    def refresh_device(self, d_rows, n, target, d_eval_rows=None, n_eval=0, eval_target=None, *, eta=0.1, reg_lambda=1.0,
                       beta=5.0, sample_weight=None, refresh_leaf=True, trace=False, stream=None):
        """refresh for the first n rows of a contiguous float32[n, n_features] matrix that lies in HBM on this model's
        device (and the first n_eval of d_eval_rows), read where they lie and complete on `stream`; labels and weights
        are host arrays.  The call returns after one synchronisation of `stream`."""
        if (d_eval_rows is None) != (eval_target is None):
            raise ValueError("d_eval_rows and eval_target go together")
        for array, rows, what in ((d_rows, n, "training"), (d_eval_rows, n_eval, "evaluation")):
            if isinstance(array, _lib.DeviceArray):
                if len(array.shape) != 2 or array.shape[1] != self.n_features or array.dtype != np.float32:
                    raise ValueError(f"the device {what} matrix must be float32[n, {self.n_features}], not "
                                     f"{array.dtype}{array.shape}")
                if isinstance(rows, (int, np.integer)) and rows > array.shape[0]:
                    raise ValueError(f"{rows} {what} rows exceed the device matrix's {array.shape[0]}")
        if d_rows is None:
            raise ValueError("the device feature matrix is missing")
        v = validate_refresh(self.n_features, None, target, None, eval_target, n=n, n_eval=n_eval, eta=eta,
                             reg_lambda=reg_lambda, beta=beta, sample_weight=sample_weight, refresh_leaf=refresh_leaf)
        return self._refresh(True, d_rows, d_eval_rows if v["n_eval"] else None, v, trace, stream)

    def _refresh(self, in_hbm, rows, eval_rows, v, trace, stream):
        """The one call behind refresh and refresh_device, after validate_refresh."""
        n, n_eval = v["n"], v["n_eval"]
        leaves = np.empty(max(self.n_nodes, 1), np.float32)[:self.n_nodes]        # never a null pointer
        node_sums = np.zeros((max(self.n_nodes, 1), 2), np.int64)[:self.n_nodes]
        margins = np.empty(n, np.float32)
        eval_errors = np.full(self.n_trees + 1, -1, np.int64)
        empty = ctypes.c_int64(0)
        probabilities = np.empty((self.n_trees, n), np.float32) if trace else None
        entry = "ds_forest_refresh_device" if in_hbm else "ds_forest_refresh"
        pointer = _lib.pointer
        _lib.check(getattr(_lib.lib(), entry)(
            self.handle, pointer(rows if n else None), n, pointer(v["target"]), pointer(v["sample_weight"]),
            pointer(eval_rows), pointer(v["eval_target"]), n_eval, v["eta"], v["reg_lambda"], v["beta"],
            int(v["refresh_leaf"]), pointer(leaves), pointer(node_sums), pointer(margins if n else None),
            pointer(eval_errors), ctypes.byref(empty), pointer(probabilities if n else None),
            *((pointer(stream),) if in_hbm else ())), entry)
        model = self._from_arrays(dict(self.arrays, threshold=leaves))
        result = RefreshResult(model, node_sums, empty.value, margins, v["reg_lambda"],
                               eval_errors if n_eval else None)
        result.trace = probabilities
        return result

    def feature_importance(self):
        """float64[n_features]: the number of splits on each feature over the sum of them (train.py
        get_xgb_feats_importance: Booster.get_fscore normalised); zeros when no tree splits."""
        splits = self.arrays["feature"]
        counts = np.bincount(splits[splits >= 0], minlength=self.n_features).astype(np.float64)
        total = counts.sum()
        return counts / total if total else counts

    def predict(self, rows, output_margin=False):
        """model.predict(xgb.DMatrix(rows)) for a host float32[n, n_features] matrix."""
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        assert rows.ndim == 2 and rows.shape[1] == self.n_features
        out = np.empty(rows.shape[0], dtype=np.float32)
        _lib.check(_lib.lib().ds_forest_predict(self.handle, _lib.pointer(rows), rows.shape[0],
                                                _lib.pointer(out if output_margin else None),
                                                _lib.pointer(None if output_margin else out)), "ds_forest_predict")
        return out

    def predict_device(self, d_rows, n, d_margins=None, d_probabilities=None, stream=None):
        pointer = _lib.pointer
        _lib.check(_lib.lib().ds_forest_predict_device(self.handle, pointer(d_rows), n, pointer(d_margins),
                                                       pointer(d_probabilities), pointer(stream)),
                   "ds_forest_predict_device")

    def calibrate_device(self, d_rows, n, d_target, stream=None):
        """calibrate for the first n rows of a float32 matrix in HBM on this model's device with its float32[n] target
        in HBM: predict_device into a probability vector that stays in HBM, then the isotonic fit there."""
        from .calibration import calibrate_rows_device
        if n and (d_rows is None or d_target is None):
            raise ValueError("the device matrix and its target are missing")
        return calibrate_rows_device(self, d_rows, n, d_target, None, stream)[0]

    def calibrate(self, rows, target):
        """What this model's probability means on labelled rows -> calibration.Calibrator: the isotonic fit of the 0/1
        labels (target != 0) on the float32 probability of every row, on the device (calibration.fit_isotonic of
        predict(rows), without the probabilities leaving HBM).  Rows the model never saw (a held-out set) give the
        honest map.  calibration.validate_calibration says what is accepted."""
        from .calibration import validate_calibration
        rows = np.asarray(rows)
        if rows.ndim != 2 or rows.shape[1] != self.n_features:
            raise ValueError(f"rows must be a [n, {self.n_features}] matrix, not shape {rows.shape}")
        if not (np.issubdtype(rows.dtype, np.floating) or np.issubdtype(rows.dtype, np.integer)):
            raise ValueError(f"rows must be numbers, not {rows.dtype}")
        v = validate_calibration(target=target, n=rows.shape[0])
        if v["target"] is None:
            raise ValueError("target is missing")
        if v["n"] == 0:
            return self.calibrate_device(None, 0, None)
        d_rows = _lib.DeviceArray.from_host(np.ascontiguousarray(rows, dtype=np.float32), self.device)
        d_target = _lib.DeviceArray.from_host(v["target"], self.device)
        try:
            return self.calibrate_device(d_rows, v["n"], d_target)
        finally:
            d_rows.free()
            d_target.free()

    def close(self):
        if self.handle:
            _lib.lib().ds_forest_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
