"""The reference's train-model step (doppelspeller/train.py): an xgboost booster trained on the construct_features
columns with the custom objective `weighted_log_loss`, early-stopped on `custom_error` of an evaluation set.

ForestTrainer grows the trees on the GPU (csrc/ds_train.hip, C ABI ds_trainer_*) by histogram gradient boosting with
depth-wise growth, the rule of xgboost's `hist` method restated in DESIGN.md ("Training"); the result is a ForestModel.
Parity with xgboost itself is unpinned, as for the forest.  The cuts are computed once per matrix: on the host
(compute_cuts) for a host matrix, on the device (compute_cuts_device, csrc/ds_cuts.hip) for a matrix that lies in HBM.

train_model(...) is the reference's one call: the training and evaluation sets from the raw titles, the booster, the
evaluation error matrix and the feature importances, with the feature matrix never leaving HBM.
"""
import concurrent.futures
import ctypes
import inspect
import time

import numpy as np

from . import _lib
from .forest import ForestModel

FEATURES_MAX = 96                      # ds_forest.hip kForestFeaturesMax: a trained model must load into ForestModel
MAX_DEPTH_MAX = 8                      # ds_train.hip kTrainMaxDepth
FALSE_POSITIVE_PENALTY_FACTOR = 5      # settings.py
PREDICTION_PROBABILITY_THRESHOLD = 0.9  # settings.py

# node states of ds_trainer_step's heap
_ABSENT, _SPLIT, _LEAF = 0, 2, 3


def feature_cuts(column, max_bin=256):
    """Cut values of one float32 column: the sorted distinct non-NaN values without the smallest when there are at most
    max_bin - 1 of them, else the distinct values of v[floor(j * n / (max_bin - 1))], j = 1 .. max_bin - 2, of the sorted
    values v (with multiplicity) that differ from v[0].  -0.0 counts as +0.0."""
    column = np.asarray(column, dtype=np.float32)
    values = np.sort(column[~np.isnan(column)] + np.float32(0.0))
    if values.shape[0] == 0:
        return np.zeros(0, np.float32)
    distinct_mask = np.empty(values.shape[0], bool)
    distinct_mask[0] = True
    np.not_equal(values[1:], values[:-1], out=distinct_mask[1:])
    if np.count_nonzero(distinct_mask) <= max_bin - 1:
        return values[distinct_mask][1:]
    n = values.shape[0]
    picks = values[(np.arange(1, max_bin - 1, dtype=np.int64) * n) // (max_bin - 1)]
    picks = np.unique(picks)
    return picks[picks != values[0]].astype(np.float32)


def compute_cuts(features, max_bin=256, threads=None):
    """(cuts float32, cut_offsets int32[n_features + 1]) of a float32[n, n_features] matrix, columns side by side on
    `threads` host threads (numpy's sort releases the GIL); the result does not depend on the thread count."""
    features = np.asarray(features, dtype=np.float32)
    columns = [features[:, f] for f in range(features.shape[1])]
    with concurrent.futures.ThreadPoolExecutor(max_workers=threads or min(16, max(1, len(columns)))) as pool:
        per_feature = list(pool.map(lambda column: feature_cuts(column, max_bin), columns))
    offsets = np.zeros(len(per_feature) + 1, np.int32)
    offsets[1:] = np.cumsum([c.shape[0] for c in per_feature])
    cuts = np.concatenate(per_feature).astype(np.float32) if per_feature else np.zeros(0, np.float32)
    return cuts, offsets


def compute_cuts_device(d_features, n, max_bin=256, n_features=None, device=None, stream=None):
    """compute_cuts of the first n rows of a contiguous float32[n, n_features] matrix in HBM (a DeviceArray, or an
    address with n_features given), sorted on the device (ds_feature_cuts_device): the same (cuts, cut_offsets), bit
    for bit.  The matrix must be complete on `stream`."""
    n_features = _device_columns(d_features, n_features)
    n = _positive_int("n", n, 1, (1 << 31) - 1)
    max_bin = _positive_int("max_bin", max_bin, 2, 256)
    if isinstance(d_features, _lib.DeviceArray) and n > d_features.shape[0]:
        raise ValueError(f"n = {n} exceeds the matrix's {d_features.shape[0]} rows")
    device = getattr(d_features, "device", 0) if device is None else device
    cuts = np.empty(n_features * 254, np.float32)
    offsets = np.empty(n_features + 1, np.int32)
    _lib.check(_lib.lib().ds_feature_cuts_device(_lib.pointer(d_features), n, n_features, max_bin, _lib.pointer(cuts),
                                                 _lib.pointer(offsets), device, _lib.pointer(stream)),
               "ds_feature_cuts_device")
    return cuts[:offsets[-1]].copy(), offsets


def cuts_option(name, value):
    """ds_cuts_option, for tests: cuts_option("column_group", g) sorts g columns at a time (0: sized from free HBM)."""
    _lib.set_option("ds_cuts_option", name, value)


def _device_columns(d_features, n_features):
    """The column count of a matrix in HBM: the DeviceArray's second dimension, or what the caller says."""
    if d_features is None:
        raise ValueError("the device feature matrix is missing")
    if n_features is None:
        shape = getattr(d_features, "shape", None)
        if shape is None or len(shape) != 2:
            raise ValueError("n_features is needed for a device matrix that is not a 2-D DeviceArray")
        n_features = shape[1]
    n_features = _positive_int("n_features", n_features)
    if n_features > FEATURES_MAX:
        raise ValueError(f"the device features have {n_features} columns, the model takes 1 to {FEATURES_MAX}")
    return n_features


def _positive_int(name, value, low=1, high=None):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < low or \
            (high is not None and value > high):
        bound = f"in [{low}, {high}]" if high is not None else f">= {low}"
        raise ValueError(f"{name} must be an integer {bound}, not {value!r}")
    return int(value)


def _real(name, value, positive=False):
    try:
        value = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a number, not {value!r}") from None
    if not np.isfinite(value) or value < 0 or (positive and value == 0):
        raise ValueError(f"{name} must be a finite {'positive' if positive else 'non-negative'} number, not {value!r}")
    return value


def _fraction(name, value):
    try:
        value = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a number in (0, 1], not {value!r}") from None
    if not 0 < value <= 1:          # refuses NaN too
        raise ValueError(f"{name} must be a number in (0, 1], not {value!r}")
    return value


SAMPLING_NAMES = ("subsample", "colsample_bytree", "colsample_bylevel", "sample_seed")

# ---- metrics of the margins ("Metrics"; csrc/ds_metrics.hip) -----------------------------------
METRIC_NAMES = ("auc", "logloss")
METRIC_FLAGS = {"auc": 1, "logloss": 2}          # DS_METRIC_AUC, DS_METRIC_LOGLOSS
LOGLOSS_QUANTUM = 1 << 20                        # a row's log loss is summed in units of 2^-20
COUNT_NAMES = ("concordant", "ties", "positives", "negatives", "logloss_sum", "rows")


def validate_metrics(metrics, what="eval_metrics"):
    """A tuple or list of distinct names from METRIC_NAMES -> the tuple, in METRIC_NAMES' order."""
    if isinstance(metrics, (str, bytes)) or not isinstance(metrics, (tuple, list)):
        raise ValueError(f"{what} must be a tuple drawn from {METRIC_NAMES}, not {metrics!r}")
    for name in metrics:
        if not isinstance(name, str) or name not in METRIC_NAMES:
            raise ValueError(f"{what} holds {name!r}; known: {METRIC_NAMES}")
    if len(set(metrics)) != len(metrics):
        raise ValueError(f"{what} names a metric twice: {metrics!r}")
    return tuple(name for name in METRIC_NAMES if name in metrics)


def metric_flags(metrics):
    return sum(METRIC_FLAGS[name] for name in metrics)


def auc_numerator(counts):
    """2 * concordant + ties: with the class sizes fixed, AUCs compare as these integers do."""
    return 2 * int(counts[0]) + int(counts[1])


def auc_value(counts):
    """(2 concordant + ties) / (2 |P| |N|) of (concordant, ties, positives, negatives, ...); NaN when a class is empty."""
    pairs = int(counts[2]) * int(counts[3])
    return auc_numerator(counts) / (2 * pairs) if pairs > 0 else float("nan")


def logloss_value(counts):
    """sum / 2^20 / rows of (..., logloss_sum, rows); NaN without rows."""
    total, rows = int(counts[-2]), int(counts[-1])
    return total / LOGLOSS_QUANTUM / rows if rows > 0 else float("nan")


def metric_values(counts, metrics):
    """{name: value} of one set's six integers (ds_trainer_metrics) for the metrics requested."""
    out = {}
    if "auc" in metrics:
        out["auc"] = auc_value(counts)
    if "logloss" in metrics:
        out["logloss"] = logloss_value(counts)
    return out


def metrics_option(name, value):
    """ds_metrics_option, for tests: metrics_option("max_blocks", b) caps the metric kernels' row grids (0: default)."""
    _lib.set_option("ds_metrics_option", name, value)


def _scores(values, what, non_empty=False):
    """The scores of auc_counts / margins of logloss_counts, checked: a 1-D float32 DeviceArray, or a host array."""
    if isinstance(values, _lib.DeviceArray):
        if len(values.shape) != 1 or values.dtype != np.float32:
            raise ValueError(f"device {what} must be a 1-D float32 DeviceArray, not {values.dtype}{values.shape}")
        return values
    values = np.asarray(values)
    if values.ndim != 1 or (non_empty and values.shape[0] < 1) or \
            not (np.issubdtype(values.dtype, np.floating) or np.issubdtype(values.dtype, np.integer)):
        raise ValueError(f"{what} must be a {'non-empty ' if non_empty else ''}1-D array of numbers, not "
                         f"{values.dtype}{values.shape}")
    return values


def auc_counts(scores, target, device=0):
    """(concordant, ties, positives, negatives, nan_rows) of float32 scores against 0/1 labels, counted on the device
    (ds_auc / ds_auc_device): scores may be a host array or a 1-D DeviceArray (then the labels are uploaded next to it).
    The order is that of the scores' integer keys: -0.0 equals +0.0, a NaN score belongs to neither class."""
    out = np.zeros(5, np.int64)
    scores = _scores(scores, "scores", non_empty=True)
    n, target = _device_labels(scores.shape[0], target, "scored")
    if isinstance(scores, _lib.DeviceArray):
        d_target = _lib.DeviceArray.from_host(target, scores.device)
        try:
            _lib.check(_lib.lib().ds_auc_device(scores.ptr, d_target.ptr, n, _lib.pointer(out), None), "ds_auc_device")
        finally:
            d_target.free()
        return tuple(int(v) for v in out)
    scores = np.ascontiguousarray(scores, dtype=np.float32)
    _lib.check(_lib.lib().ds_auc(_lib.pointer(scores), _lib.pointer(target), n, _lib.pointer(out), device), "ds_auc")
    return tuple(int(v) for v in out)


def logloss_counts(margins, target, beta=5.0, device=0):
    """(fixed-point sum, rows) of the weighted log loss of float32 margins against 0/1 labels, summed on the device
    (ds_weighted_logloss_device); margins may be a host array or a 1-D float32 DeviceArray.  logloss_value gives
    sum / 2^20 / rows."""
    beta = _real("beta", beta, positive=True)
    margins = _scores(margins, "margins")
    on_device = isinstance(margins, _lib.DeviceArray)
    if on_device:
        device = margins.device
    n, target = _device_labels(margins.shape[0], target, "scored")
    d_margins = margins if on_device else _lib.DeviceArray.from_host(margins.astype(np.float32), device)
    d_target = _lib.DeviceArray.from_host(target, device)
    out = np.zeros(2, np.int64)
    try:
        _lib.check(_lib.lib().ds_weighted_logloss_device(d_margins.ptr, d_target.ptr, n, beta, _lib.pointer(out), None),
                   "ds_weighted_logloss_device")
    finally:
        d_target.free()
        if not on_device:
            d_margins.free()
    return int(out[0]), int(out[1])


def roc_auc(scores, target, device=0):
    """The area under the ROC curve of auc_counts(scores, target): NaN when a class is empty."""
    return auc_value(auc_counts(scores, target, device))


def _labels(n, target, what):
    """One 0/1 label for each of the n `what` rows -> float32[n]."""
    target = np.asarray(target)
    if target.ndim != 1 or target.shape[0] != n:
        raise ValueError(f"{n} {what} rows but {target.reshape(-1).shape[0]} labels")
    if target.dtype == object or not np.isin(target, (0, 1)).all():
        raise ValueError(f"{what} labels must all be 0 or 1")
    return np.ascontiguousarray(target, dtype=np.float32)


def _device_labels(n, target, what):
    n = _positive_int(f"the number of {what} rows", n, 1, (1 << 31) - 1)
    return n, _labels(n, target, what)


def _matrix_and_labels(features, target, what):
    features = np.asarray(features)
    if features.ndim != 2:
        raise ValueError(f"{what} features must be a 2-D matrix, not shape {features.shape}")
    if not (np.issubdtype(features.dtype, np.floating) or np.issubdtype(features.dtype, np.integer)):
        raise ValueError(f"{what} features must be numbers, not {features.dtype}")
    if features.shape[0] < 1:
        raise ValueError(f"{what} features need at least one row")
    if not 1 <= features.shape[1] <= FEATURES_MAX:
        raise ValueError(f"{what} features have {features.shape[1]} columns, the model takes 1 to {FEATURES_MAX}")
    target = _labels(features.shape[0], target, what)
    return np.ascontiguousarray(features, dtype=np.float32), target


def validate_fit(features, target, eval_features=None, eval_target=None, **parameters):
    """fit's checks (no library needed) -> (features, target, eval_features, eval_target, params) as float32 arrays.
    parameters: validate_parameters' own, by keyword; a name it does not know is its TypeError."""
    features, target = _matrix_and_labels(features, target, "training")
    if (eval_features is None) != (eval_target is None):
        raise ValueError("eval_features and eval_target go together")
    if eval_features is not None:
        eval_features, eval_target = _matrix_and_labels(eval_features, eval_target, "evaluation")
        if eval_features.shape[1] != features.shape[1]:
            raise ValueError(f"evaluation features have {eval_features.shape[1]} columns, training features "
                             f"{features.shape[1]}")
    return features, target, eval_features, eval_target, validate_parameters(**parameters)


def validate_parameters(num_boost_round=1000, early_stopping_rounds=50, max_depth=5, eta=0.1, min_child_weight=1.0,
                        reg_lambda=1.0, beta=5.0, max_bin=256, subsample=1.0, colsample_bytree=1.0,
                        colsample_bylevel=1.0, sample_seed=0, eval_metrics=()):
    """The booster parameters, checked -> params.  This signature is the ONE list of their names and defaults:
    validate_fit, validate_fit_device and ForestTrainer's begin and fit forms take them as **parameters and hand them
    here, tuning and train_model read the names from it.  subsample, colsample_bytree and colsample_bylevel are
    fractions in (0, 1] ("Subsampling"); sample_seed in [0, 2^63) seeds their draws and is not the
    `seed` of the training set and the folds.  eval_metrics: a tuple drawn from METRIC_NAMES, reported per round
    ("Metrics"); it changes no tree."""
    params = dict(num_boost_round=_positive_int("num_boost_round", num_boost_round),
                  early_stopping_rounds=_positive_int("early_stopping_rounds", early_stopping_rounds),
                  max_depth=_positive_int("max_depth", max_depth, 1, MAX_DEPTH_MAX),
                  eta=_real("eta", eta, positive=True), min_child_weight=_real("min_child_weight", min_child_weight),
                  reg_lambda=_real("reg_lambda", reg_lambda), beta=_real("beta", beta, positive=True),
                  max_bin=_positive_int("max_bin", max_bin, 2, 256),
                  subsample=_fraction("subsample", subsample),
                  colsample_bytree=_fraction("colsample_bytree", colsample_bytree),
                  colsample_bylevel=_fraction("colsample_bylevel", colsample_bylevel),
                  sample_seed=_positive_int("sample_seed", sample_seed, 0, (1 << 63) - 1),
                  eval_metrics=validate_metrics(eval_metrics))
    if params["reg_lambda"] == 0 and params["min_child_weight"] == 0:
        raise ValueError("reg_lambda and min_child_weight cannot both be 0 (an empty child would divide by zero)")
    if params["reg_lambda"] == 0 and params["subsample"] < 1:
        raise ValueError("subsample < 1 needs reg_lambda > 0 (a round that draws no row would divide by zero)")
    return params


def validate_init_model(init_model, n_features, device=None):
    """The checks of an `init_model` argument (no device work) -> the model.  It must be an open ForestModel with the
    matrix's n_features and base margin 0 -- base_score 0.5, the trainer's own, which ForestTrainer's models and
    xgboost imports with the default base_score have -- and, when `device` is given, live on that device.  Its depth
    and tree count are free; a model of zero trees is legal ("Continuing from a model")."""
    if not isinstance(init_model, ForestModel):
        raise ValueError(f"init_model must be a ForestModel, not {type(init_model).__name__}")
    if not init_model.handle:
        raise ValueError("init_model is closed")
    if init_model.n_features != n_features:
        raise ValueError(f"init_model has {init_model.n_features} features, the training features {n_features}")
    if init_model.arrays["base_margin"] != 0.0:
        raise ValueError(f"init_model has base margin {init_model.arrays['base_margin']!r}; training continues only from "
                         "base margin 0 (base_score 0.5)")
    if device is not None and init_model.device != device:
        raise ValueError(f"init_model lives on device {init_model.device}, the trainer on device {device}")
    return init_model


WEIGHT_GUARD = float(1 << 32)           # ds_train.hip train_check_weights: max(beta, 1) * sum(weights) at most


def validate_sample_weight(sample_weight, n, beta=5.0):
    """The checks of a `sample_weight` argument (no library needed) -> contiguous float32[n] (DESIGN.md section 9,
    "Sample weights").  One weight per training row: a 1-D array of n numbers, every one finite and >= 0 AS A FLOAT32
    (what the device multiplies by), with a total above 0 and max(beta, 1) * total <= 2^32, the total taken in float64:
    the bound that keeps the trainer's int64 sums from overflowing.  For a batch, beta is the largest of its models.
    A weight scales the row's gradient and hessian and nothing else: not the cuts (compute_cuts and
    compute_cuts_device see values alone), not the subsample draw (indexed by row number), not the evaluation error,
    initial_error(s) or early stopping, not eval_metrics / metrics (counts over rows), not fit_cover (counts rows)."""
    weights = np.asarray(sample_weight)
    if weights.ndim != 1:
        raise ValueError(f"sample_weight must be a 1-D array, not shape {weights.shape}")
    if weights.shape[0] != n:
        raise ValueError(f"{n} training rows but {weights.shape[0]} sample weights")
    if weights.dtype == bool or not (np.issubdtype(weights.dtype, np.floating) or
                                      np.issubdtype(weights.dtype, np.integer)):
        raise ValueError(f"sample_weight must hold numbers, not {weights.dtype}")
    with np.errstate(over="ignore"):
        weights = np.ascontiguousarray(weights, dtype=np.float32)
    if not np.isfinite(weights).all():
        raise ValueError("sample_weight holds a NaN or an infinite value (as float32)")
    if (weights < 0).any():
        raise ValueError(f"sample_weight holds a negative value (row {int(np.argmax(weights < 0))})")
    total = float(weights.astype(np.float64).sum())
    if not total > 0:
        raise ValueError("the total sample weight of the training rows is 0")
    if max(float(beta), 1.0) * total > WEIGHT_GUARD:
        raise ValueError(f"max(beta, 1) * the total sample weight = {max(float(beta), 1.0) * total!r} exceeds 2^32: the "
                         "trainer's integer sums could overflow (scale the weights down)")
    return weights


def validate_monotone_constraints(constraints, n_features, feature_names=None):
    """The checks of a `monotone_constraints` argument (no library needed) -> contiguous int8[n_features] (DESIGN.md
    section 9, "Monotone constraints"; xgboost's monotone_constraints).  Either a 1-D sequence of n_features integers,
    each -1 (the prediction never rises with the feature), 0 (free) or +1 (it never falls): bools, floats that are not
    whole and NaN are refused, a wrong length by name.  Or, when `feature_names` names the n_features columns, a dict
    {feature name: sign}, a name left out being 0; an unknown name is refused, listing it."""
    def sign(value, what):
        if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, float, np.integer, np.floating)) or \
                value not in (-1, 0, 1):          # NaN and 0.5 are in no tuple; 1.0 is
            raise ValueError(f"monotone_constraints: {what} must be -1, 0 or 1, not {value!r}")
        return int(value)

    out = np.zeros(n_features, np.int8)
    if isinstance(constraints, dict):
        if feature_names is None:
            raise ValueError("monotone_constraints by name (a dict) needs the feature names; give a sequence of "
                             f"{n_features} signs")
        names = list(feature_names)
        if len(names) != n_features:
            raise ValueError(f"monotone_constraints: {len(names)} feature names for {n_features} features")
        unknown = sorted(str(name) for name in constraints if name not in names)
        if unknown:
            raise ValueError(f"monotone_constraints names unknown features {unknown}")
        for name, value in constraints.items():
            out[names.index(name)] = sign(value, f"the sign of {name!r}")
        return out
    if isinstance(constraints, (str, bytes)) or not isinstance(constraints, (list, tuple, np.ndarray)):
        raise ValueError(f"monotone_constraints must be a 1-D sequence of {n_features} signs or a dict by feature "
                         f"name, not {constraints!r}")
    if isinstance(constraints, np.ndarray) and constraints.ndim != 1:
        raise ValueError(f"monotone_constraints must be 1-D, not shape {constraints.shape}")
    if len(constraints) != n_features:
        raise ValueError(f"{n_features} features but {len(constraints)} monotone_constraints")
    if isinstance(constraints, np.ndarray) and (constraints.dtype == bool or not (
            np.issubdtype(constraints.dtype, np.integer) or np.issubdtype(constraints.dtype, np.floating))):
        raise ValueError(f"monotone_constraints must hold -1, 0 or 1, not {constraints.dtype}")
    for f, value in enumerate(constraints):
        out[f] = sign(value, f"entry {f}")
    return out


def _samples(params):
    """Whether a parameter set draws rows or columns: a fraction below 1 (a set that carries none draws nothing)."""
    return any(params.get(name, 1.0) < 1 for name in SAMPLING_NAMES[:3])


def validate_fit_device(d_features, n, target, d_eval_features=None, n_eval=0, eval_target=None, *, n_features=None,
                        **parameters):
    """fit_device's checks (no library needed) -> (n, target, n_eval, eval_target, n_features, params): validate_fit
    for matrices in HBM, of which only the shapes are known here."""
    n_features = _device_columns(d_features, n_features)
    n, target = _device_labels(n, target, "training")
    if (d_eval_features is None) != (eval_target is None):
        raise ValueError("d_eval_features and eval_target go together")
    if d_eval_features is not None:
        columns = _device_columns(d_eval_features, n_features if getattr(d_eval_features, "shape", None) is None
                                  else None)
        if columns != n_features:
            raise ValueError(f"evaluation features have {columns} columns, training features {n_features}")
        n_eval, eval_target = _device_labels(n_eval, eval_target, "evaluation")
    else:
        n_eval = 0
    for array, rows, what in ((d_features, n, "training"), (d_eval_features, n_eval, "evaluation")):
        if isinstance(array, _lib.DeviceArray) and rows > array.shape[0]:
            raise ValueError(f"{rows} {what} rows exceed the device matrix's {array.shape[0]}")
    return n, target, n_eval, eval_target, n_features, validate_parameters(**parameters)


def heap_tree(info, leaf, cuts, cut_offsets):
    """Heap-ordered nodes of ds_trainer_step / ds_trainer_batch_step -> ForestModel arrays of one tree (breadth-first
    ids: children after their parent).  Slots beyond the tree's own depth are absent and never visited."""
    order, ids = [0], {0: 0}
    for node in order:
        if info[node, 0] == _SPLIT:
            for child in (2 * node + 1, 2 * node + 2):
                ids[child] = len(order)
                order.append(child)
    size = len(order)
    tree = dict(feature=np.full(size, -1, np.int32), threshold=np.zeros(size, np.float32),
                yes=np.zeros(size, np.int32), no=np.zeros(size, np.int32), missing=np.zeros(size, np.int32))
    for i, node in enumerate(order):
        state, feature, bin_, default_left = (int(v) for v in info[node])
        if state == _SPLIT:
            left, right = ids[2 * node + 1], ids[2 * node + 2]
            tree["feature"][i] = feature
            tree["threshold"][i] = cuts[cut_offsets[feature] + bin_ - 1]   # bins < b  <=>  x < cut
            tree["yes"][i], tree["no"][i] = left, right
            tree["missing"][i] = left if default_left else right
        else:
            assert state == _LEAF, f"node {node}: state {state}"
            tree["threshold"][i] = leaf[node]
    return tree


class FirstMinimum:
    """The stopping rule of every training loop (ForestTrainer.fit, cross_validate, select_parameters): `best` is the
    round of the FIRST minimum of the values seen, `value` that minimum; see(round_, value) says whether the loop stops
    after this round, which it does once round_ - best >= patience (None: never)."""

    def __init__(self, patience=None):
        self.patience, self.best, self.value = patience, None, None

    def see(self, round_, value):
        if self.best is None or value < self.value:
            self.best, self.value = round_, value
        return self.patience is not None and round_ - self.best >= self.patience


def _call(entry, in_hbm, *arguments):
    """One checked call of a library entry that has a form for a matrix in HBM, named `<entry>_device`."""
    entry += "_device" if in_hbm else ""
    _lib.check(getattr(_lib.lib(), entry)(*arguments), entry)


def _step_form(parameters):
    """begin and begin_device grow no round: to them the two round names are unknown names."""
    for name in ("num_boost_round", "early_stopping_rounds"):
        if name in parameters:
            raise TypeError(f"begin and begin_device got an unexpected keyword argument {name!r}")
    return parameters


class _TrainerHandle:
    """What ForestTrainer and ForestTrainerBatch (tuning.py) do alike with their library object.  ENTRIES is the prefix
    of its entries' names, READS the buffers of its read entry in argument order."""
    ENTRIES, READS = None, ()

    def _model(self, trees, n_trees):
        """ForestModel of the first n_trees of `trees` (None: all), after the init model's if there is one."""
        trees = trees[:len(trees) if n_trees is None else n_trees]
        if self.init_model is not None:
            return self.init_model.extended(trees)
        return ForestModel.from_trees(trees, self.n_features, device=self.device)

    def _set_metrics(self, metrics, rows):
        """The buffer that every step's counts are read into (`rows` sets or models) and the metrics to the library,
        once the labels and the held-out rows are in place (none: nothing to set)."""
        self._metric_counts = np.full((rows, 6), -1, np.int64)
        if metrics:
            _lib.check(getattr(_lib.lib(), self.ENTRIES + "_set_metrics")(self.handle, metric_flags(metrics)),
                       self.ENTRIES + "_set_metrics")

    def _read(self, *model, **wanted):
        """{name: array} of the device buffers wanted, each given as name=(shape, dtype); `model`: the batch's index."""
        out = {name: np.empty(shape, dtype) for name, (shape, dtype) in wanted.items()}
        _lib.check(getattr(_lib.lib(), self.ENTRIES + "_read")(
            self.handle, *(int(m) for m in model), *(_lib.pointer(out.get(name)) for name in self.READS)),
            self.ENTRIES + "_read")
        return out

    def close(self):
        if self.handle:
            getattr(_lib.lib(), self.ENTRIES + "_destroy")(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ForestTrainer(_TrainerHandle):
    """xgb.train(params={max_depth, eta, min_child_weight, subsample, colsample_bytree, colsample_bylevel},
    obj=weighted_log_loss, feval=custom_error, early_stopping_rounds) on the GPU.

        model = ForestTrainer().fit(features, target, eval_features, eval_target, max_depth=5, eta=0.1)

    The data arguments may be given by position; the booster parameters (validate_parameters: its signature is their
    list and their defaults), `init_model`, `sample_weight`, `monotone_constraints` and the device forms' `n_features` by
    keyword ONLY.  fit
    and fit_device take all of them; begin and begin_device all but num_boost_round and early_stopping_rounds.  A name that
    validate_parameters does not know is a TypeError.  Everything is validated, once, before the library is touched,
    and a trainer whose begin or fit is refused keeps the state it had.

    After fit, `best_iteration` is the round (from 0) of the first minimum of the evaluation error and `history` the
    error of every round; the model holds the first best_iteration + 1 trees (the reference predicts with
    ntree_limit=best_ntree_limit).  Without an evaluation set every round is kept.  The step form: begin(...), then
    step() grows one tree and returns the round's evaluation error (None without an evaluation set).  `timings` has the
    milliseconds of the last begin: "cuts", and "bin" for everything from the trainer's creation to its metrics.

    eval_metrics=("auc", "logloss") also reports, per round, the reference's log: `metrics_history` gains one value per
    key "train-auc", "evaluation-auc", "train-logloss", "evaluation-logloss" (evaluation keys only with an evaluation
    set) and `metric_counts` the integers they come from ({"train": (concordant, ties, positives, negatives,
    logloss_sum, rows), "evaluation": ...} per round, -1 for a metric not requested).  They are computed on the device
    from the margins of ALL rows of a set and change neither the trees nor the early stopping.

    init_model=<ForestModel> continues boosting from that model (xgb.train(..., xgb_model=booster); DESIGN.md section 9,
    "Continuing from a model"): the margins start at the model's, evaluated on the raw features on the device, and the
    new trees are those a trainer would grow that had grown the model's trees itself.  `trees` and `history` hold the
    NEW rounds, `initial_error` the evaluation error of the init model (None without an evaluation set), model(n) the
    init trees followed by the first n new ones.  Early stopping looks at the new rounds only (the first minimum of
    `history`; initial_error is no candidate), and `best_iteration` counts all trees: init trees + the best new round,
    so that the model returned has best_iteration + 1 trees as ever.  See validate_init_model for what is accepted.

    sample_weight=<array of n numbers> weighs the training rows in the objective (xgb.DMatrix(weight=...); DESIGN.md
    section 9, "Sample weights"): a row's gradient and hessian are multiplied by its weight before they are quantized,
    so min_child_weight bounds a sum of weighted hessians and a row of weight 0 trains nothing.  It is data, like the
    labels, a host array for all four forms, and is kept as `sample_weight` (float32, None without).  The weights do
    NOT touch the cuts, the `subsample` draw (indexed by row number), the evaluation error, `initial_error`, early
    stopping, `eval_metrics` (counts over rows) or ForestModel.fit_cover (counts rows).  See validate_sample_weight
    for what is accepted; all weights 1 grows the trees of a call without the argument, bit for bit.

    monotone_constraints=<n_features signs> makes every new tree, and so the forest's margin, monotone in the features
    it names (xgboost's monotone_constraints; DESIGN.md section 9, "Monotone constraints"): +1 never falls as the
    feature rises, -1 never rises, 0 is free.  The split choice rejects candidates whose children stand in the wrong
    order and clamps weights to the bounds a constrained split leaves its children; cuts, gradients, draws, errors,
    metrics and cover are untouched.  It is kept as `monotone_constraints` (int8, None without); None or all zeros makes
    exactly the calls of a trainer that knows no constraints.  With init_model the NEW trees are constrained, the init
    trees are what they are.  ForestModel.monotone_violations(constraints) counts the splits that break it: 0 for every
    model grown here.  See validate_monotone_constraints for what is accepted."""
    ENTRIES, READS = "ds_trainer", ("margins", "probabilities", "gradients", "bins", "eval_margins")

    def __init__(self, device=0):
        self.device = device
        self.handle = None
        self.trees = []
        self.history = []
        self.best_iteration = None
        self.init_model = None
        self.initial_error = None
        self.sample_weight = None
        self.monotone_constraints = None
        self.eval_metrics = ()
        self.metrics_history = {}
        self.metric_counts = []

    def begin(self, features, target, eval_features=None, eval_target=None, **parameters):
        return self._begin(False, (features, target, eval_features, eval_target), **_step_form(parameters))

    def fit(self, features, target, eval_features=None, eval_target=None, **parameters):
        self._begin(False, (features, target, eval_features, eval_target), **parameters)
        return self._boost(self.params)

    def begin_device(self, d_features, n, target, d_eval_features=None, n_eval=0, eval_target=None, **parameters):
        """begin for matrices that already lie in HBM: contiguous float32[n, n_features] DeviceArrays (or addresses,
        with n_features given), complete before the call; labels are host arrays.  The cuts come from
        compute_cuts_device, the bins from the same kernel as begin's, so every later call works as after begin.  The
        matrices are not kept and may be freed afterwards."""
        return self._begin(True, (d_features, n, target, d_eval_features, n_eval, eval_target),
                           **_step_form(parameters))

    def fit_device(self, d_features, n, target, d_eval_features=None, n_eval=0, eval_target=None, **parameters):
        """fit for matrices in HBM (begin_device, then fit's rounds and early stopping)."""
        self._begin(True, (d_features, n, target, d_eval_features, n_eval, eval_target), **parameters)
        return self._boost(self.params)

    def _begin(self, in_hbm, data, init_model=None, sample_weight=None, monotone_constraints=None, **parameters):
        """The one sequence behind the four forms above; `data` are their data arguments.  Everything is validated
        first: until that has passed the library is not touched and this trainer keeps the state it has."""
        if in_hbm:
            n, target, n_eval, eval_target, n_features, params = validate_fit_device(*data, **parameters)
            features, eval_features = data[0], data[3]
        else:
            features, target, eval_features, eval_target, params = validate_fit(*data, **parameters)
            (n, n_features), n_eval = features.shape, 0 if eval_features is None else eval_features.shape[0]
        if init_model is not None:
            validate_init_model(init_model, n_features, self.device)
        if sample_weight is not None:
            sample_weight = validate_sample_weight(sample_weight, n, params["beta"])
        if monotone_constraints is not None:
            monotone_constraints = validate_monotone_constraints(monotone_constraints, n_features)
        self.close()
        self.params = params
        self.sample_weight = sample_weight
        self.monotone_constraints = monotone_constraints
        self.n, self.n_features, self.n_eval = n, n_features, n_eval
        self.timings = {}
        mark = time.perf_counter()
        self.cuts, self.cut_offsets = compute_cuts_device(features, n, params["max_bin"], n_features, self.device) \
            if in_hbm else compute_cuts(features, params["max_bin"])
        self.timings["cuts"] = (time.perf_counter() - mark) * 1000.0
        self.trees, self.history, self.best_iteration = [], [], None
        mark = time.perf_counter()
        handle = ctypes.c_void_p()
        _call("ds_trainer_create", in_hbm, _lib.pointer(features), n, n_features, _lib.pointer(self.cuts),
              _lib.pointer(self.cut_offsets), params["max_depth"], params["eta"], params["min_child_weight"],
              params["reg_lambda"], params["beta"], self.device, ctypes.byref(handle))
        self.handle = handle
        library = _lib.lib()
        if _samples(params):                   # all fractions 1: nothing to set
            _lib.check(library.ds_trainer_set_sampling(self.handle, params["subsample"], params["colsample_bytree"],
                                                       params["colsample_bylevel"], params["sample_seed"]),
                       "ds_trainer_set_sampling")
        _lib.check(library.ds_trainer_set_labels(self.handle, _lib.pointer(target)), "ds_trainer_set_labels")
        if sample_weight is not None:          # none: exactly the calls of a trainer that knows no weights
            _lib.check(library.ds_trainer_set_weights(self.handle, _lib.pointer(sample_weight)),
                       "ds_trainer_set_weights")
        if monotone_constraints is not None and monotone_constraints.any():   # none or all zeros: nothing to set
            _lib.check(library.ds_trainer_set_monotone(self.handle, _lib.pointer(monotone_constraints)),
                       "ds_trainer_set_monotone")
        if n_eval:
            _call("ds_trainer_set_eval", in_hbm, self.handle, _lib.pointer(eval_features), _lib.pointer(eval_target),
                  n_eval)
        self.init_model, self.initial_error = init_model, None
        if init_model is not None:             # the margins start from it, now that labels and evaluation set are in
            error = ctypes.c_int64(-1)
            _call("ds_trainer_seed", in_hbm, self.handle, init_model.handle, _lib.pointer(features),
                  _lib.pointer(eval_features), ctypes.byref(error), *((None,) if in_hbm else ()))
            self.initial_error = int(error.value) if n_eval else None
        self.eval_metrics = params["eval_metrics"]
        sets = ("train", "evaluation") if n_eval else ("train",)
        self.metrics_history = {f"{set_}-{metric}": [] for metric in self.eval_metrics for set_ in sets}
        self.metric_counts = []
        self._set_metrics(self.eval_metrics, 2)
        self.timings["bin"] = (time.perf_counter() - mark) * 1000.0
        slots = (2 << params["max_depth"]) - 1
        self._info = np.zeros((slots, 4), np.int32)
        self._leaf = np.zeros(slots, np.float32)
        return self

    def step(self):
        """Grow one tree; returns the evaluation error after it (None without an evaluation set)."""
        if not self.handle:
            raise RuntimeError("ForestTrainer.step before begin")
        error = ctypes.c_int64(-1)
        _lib.check(_lib.lib().ds_trainer_step(self.handle, _lib.pointer(self._info), _lib.pointer(self._leaf),
                                              ctypes.byref(error)), "ds_trainer_step")
        self.last_heap = (self._info.copy(), self._leaf.copy())   # ds_trainer_step's heap order, for tests
        self.trees.append(self._tree(self._info, self._leaf))
        value = int(error.value) if self.n_eval else None
        self.history.append(value)
        if self.eval_metrics:
            _lib.check(_lib.lib().ds_trainer_metrics(self.handle, _lib.pointer(self._metric_counts)),
                       "ds_trainer_metrics")
            sets = ("train", "evaluation") if self.n_eval else ("train",)
            self.metric_counts.append({set_: tuple(int(v) for v in self._metric_counts[i])
                                       for i, set_ in enumerate(sets)})
            for i, set_ in enumerate(sets):
                for metric, number in metric_values(self._metric_counts[i], self.eval_metrics).items():
                    self.metrics_history[f"{set_}-{metric}"].append(number)
        return value

    def _tree(self, info, leaf):
        """Heap-ordered nodes -> ForestModel arrays of one tree (heap_tree with this trainer's cuts)."""
        return heap_tree(info, leaf, self.cuts, self.cut_offsets)

    def model(self, n_trees=None):
        """ForestModel of the first n_trees trees grown here (default: all so far), after the init model's if there is
        one."""
        return self._model(self.trees, n_trees)

    def _boost(self, rounds):
        """Step up to rounds["num_boost_round"] times under FirstMinimum(rounds["early_stopping_rounds"]) on the
        evaluation error -> the model of the best round's trees."""
        rule = FirstMinimum(rounds["early_stopping_rounds"])
        for round_ in range(rounds["num_boost_round"]):
            error = self.step()
            if error is not None and rule.see(round_, error):
                break
        best = rule.best if rule.best is not None else len(self.trees) - 1   # no evaluation set: every round is kept
        self.best_iteration = (self.init_model.n_trees if self.init_model is not None else 0) + best
        return self.model(best + 1)

    def margins(self):
        """Training margins after the trees so far (float32[n])."""
        return self._read(margins=(self.n, np.float32))["margins"]

    def eval_margins(self):
        return self._read(eval_margins=(self.n_eval, np.float32))["eval_margins"]

    def probabilities(self):
        """The float32 probabilities the last step took its gradients at."""
        return self._read(probabilities=(self.n, np.float32))["probabilities"]

    def gradients(self):
        """int64[n, 2]: the last step's quantized (gradient, hessian), rint(x * 2^30)."""
        return self._read(gradients=((self.n, 2), np.int64))["gradients"]

    def bins(self):
        """uint8[n_features, n]: the device's bins (255 = missing)."""
        return self._read(bins=((self.n_features, self.n), np.uint8))["bins"]


def evaluation_error_matrix(model, features, target, threshold=PREDICTION_PROBABILITY_THRESHOLD):
    """(true positives, true negatives, false positives, false negatives) of the model's predictions at `threshold`
    (train.py:get_evaluation_error_matrix)."""
    return _error_matrix(model.predict(np.ascontiguousarray(features, dtype=np.float32)), target, threshold)


def _error_matrix(probabilities, target, threshold):
    # train.py:65-66 compares the booster's float32 predictions with a Python float, which NumPy does in float32; a
    # threshold that arrives as a NumPy float64 must not turn that into a float64 compare
    predicted = np.asarray(probabilities, dtype=np.float32) > np.float32(threshold)
    actual = np.asarray(target).reshape(-1) != 0
    return (int(np.count_nonzero(predicted & actual)), int(np.count_nonzero(~predicted & ~actual)),
            int(np.count_nonzero(predicted & ~actual)), int(np.count_nonzero(~predicted & actual)))


class TrainModelResult:
    """What train_model returns: `model` (ForestModel of best_iteration + 1 trees), `feature_importance` (the
    reference's return value: ForestModel.feature_importance()), `error_matrix` ((tp, tn, fp, fn) on the evaluation set
    at 0.9, what the reference logs; None without an evaluation set), `best_iteration`, `history`, `rows` (the
    DataFrame of FeatureEngineering.rows), `timings` (milliseconds per stage, "total" for the call) and, when
    eval_metrics were requested, `metrics_history` (ForestTrainer.metrics_history; None otherwise).  With init_model:
    `initial_error`, the evaluation error of the init model (None otherwise and without an evaluation set); `model`,
    `feature_importance` and a counted cover are those of the WHOLE forest, `history` that of the new rounds and
    `best_iteration` counts all trees (ForestTrainer).  With permutation_repeats > 0: `permutation_importance`, the
    model's PermutationImportance on the evaluation set (None otherwise).  With bootstrap_repeats > 0:
    `error_bootstrap`, the ErrorBootstrap of the model (and of the init model) on the evaluation set (None otherwise).
    With calibrate=True: `calibrator`, the Calibrator of the model's probability on the evaluation set, `reliability`,
    the ReliabilityReport of the raw probability there, and `calibrated_reliability`, that of the calibrated value (all
    three None otherwise).  With misspelling_profile: `misspelling_profile`, the MisspellingProfile the generated rows
    followed (the fitted one for "fit"; None otherwise)."""

    def __init__(self, model, feature_importance, error_matrix, best_iteration, history, rows, timings,
                 metrics_history=None, initial_error=None, permutation_importance=None, error_bootstrap=None,
                 calibrator=None, reliability=None, calibrated_reliability=None, misspelling_profile=None):
        self.model, self.feature_importance, self.error_matrix = model, feature_importance, error_matrix
        self.best_iteration, self.history, self.rows, self.timings = best_iteration, history, rows, timings
        self.metrics_history = metrics_history
        self.initial_error = initial_error
        self.permutation_importance = permutation_importance
        self.error_bootstrap = error_bootstrap
        self.calibrator, self.reliability, self.calibrated_reliability = calibrator, reliability, calibrated_reliability
        self.misspelling_profile = misspelling_profile


def refresh_model(truth_titles, truth_title_ids, train_titles, train_title_ids, model, top_n=100, sample_n=10, seed=0,
                  device=0, transform=True, evaluation_fractions=None, build_index="host", kind_weights=None, eta=0.1,
                  reg_lambda=1.0, beta=5.0, refresh_leaf=True, misspelling_profile=None):
    """ForestModel.refresh from raw titles: FeatureEngineering(...).generate_device_data_sets(), the device data sets
    train_model trains on, then model.refresh_device on the training matrix where it lies in HBM, with the evaluation
    matrix (when the fractions draw one) for the errors per tree prefix.  The feature matrices never leave HBM.
    model: an open ForestModel of FEATURES_COUNT features on `device`; it is not modified.  kind_weights: as
    train_model's, the sample weight of the training rows by kind, handed on as sample_weight.  eta, reg_lambda, beta,
    refresh_leaf: ForestModel.refresh's.  misspelling_profile: FeatureEngineering's (None, a MisspellingProfile or
    "fit").  Everything is validated before any device work.  Returns the RefreshResult with more attributes: `rows`
    (the DataFrame of FeatureEngineering.rows), `timings` (milliseconds per stage of the data sets, "refresh" and
    "total") and `misspelling_profile` (the profile the generated rows followed, None without one)."""
    from .feature_engineering import FEATURES_COUNT
    from .forest import validate_refresh
    from .training_set import FeatureEngineering, kind_weights as weights_of_kinds, validate_kind_weights
    started = time.perf_counter()
    if not isinstance(model, ForestModel):
        raise ValueError(f"model must be a ForestModel, not {type(model).__name__}")
    if not model.handle:
        raise ValueError("model is closed")
    if model.n_features != FEATURES_COUNT:
        raise ValueError(f"model has {model.n_features} features, the title features are {FEATURES_COUNT}")
    if model.device != device:
        raise ValueError(f"model lives on device {model.device}, the data sets on device {device}")
    validate_refresh(FEATURES_COUNT, None, np.zeros(1, np.float32), n=1, eta=eta, reg_lambda=reg_lambda, beta=beta,
                     refresh_leaf=refresh_leaf)
    if kind_weights is not None:
        validate_kind_weights(kind_weights)
    fe = FeatureEngineering(truth_titles, truth_title_ids, train_titles, train_title_ids, top_n=top_n,
                            sample_n=sample_n, seed=seed, device=device, transform=transform,
                            evaluation_fractions=evaluation_fractions, build_index=build_index,
                            misspelling_profile=misspelling_profile)
    sets = fe.generate_device_data_sets()
    timings = dict(fe.timings)
    has_eval = sets.n_evaluation > 0
    weighted = {} if kind_weights is None else dict(sample_weight=weights_of_kinds(fe.rows, kind_weights))
    mark = time.perf_counter()
    try:
        result = model.refresh_device(sets.train, sets.n_train, sets.train_target,
                                      sets.evaluation if has_eval else None, sets.n_evaluation,
                                      sets.evaluation_target if has_eval else None, eta=eta, reg_lambda=reg_lambda,
                                      beta=beta, refresh_leaf=refresh_leaf, **weighted)
    finally:
        sets.free()
    timings["refresh"] = (time.perf_counter() - mark) * 1000.0
    timings["total"] = (time.perf_counter() - started) * 1000.0
    result.rows, result.timings, result.misspelling_profile = fe.rows, timings, fe.misspelling_profile
    return result


def train_model(truth_titles, truth_title_ids, train_titles, train_title_ids, top_n=100, sample_n=10, seed=0, device=0,
                transform=True, evaluation_fractions=None, cover=False, build_index="host", init_model=None,
                kind_weights=None, monotone_constraints=None, permutation_repeats=0, permutation_seed=0,
                bootstrap_repeats=0, bootstrap_seed=0, calibrate=False, reliability_bins=10, misspelling_profile=None,
                **fit_parameters):
    """train.train_model() of the reference in one call: FeatureEngineering(...).generate_device_data_sets() ->
    ForestTrainer.fit_device -> the evaluation error matrix (ForestModel.predict_device on the evaluation matrix in
    HBM, only its probabilities come back) and the feature importances.  The feature matrix never leaves HBM.
    fit_parameters: those of ForestTrainer.fit (num_boost_round, early_stopping_rounds, max_depth, eta, ...,
    eval_metrics=("auc", "logloss") for the reference's per-round train-auc / evaluation-auc log).
    Everything is validated before any device work.  Evaluation fractions of 0 for all three kinds train without an
    evaluation set: every round is kept and error_matrix is None.
    cover: also count the training matrix through the finished trees while it is still in HBM
    (ForestModel.fit_cover_device), so that the returned model can explain its predictions
    (predict_contributions, Prediction.explain); `timings` then has a "cover" entry.  The trees are the same either
    way.  build_index: "host" or "device", where the truth index is built (TruthSide).
    init_model: a ForestModel of FEATURES_COUNT features to continue from (ForestTrainer; validate_init_model): the
    device chain is the same, seeded from the matrices in HBM, and the result gains `initial_error`.
    kind_weights: {"generated", "negative", "positive"} -> the sample weight of the training rows of that kind (a name
    left out: 1.0; training_set.kind_weights), handed to fit_device as sample_weight.  The weights enter the objective
    alone (ForestTrainer): the evaluation error, error_matrix and a counted cover stay counts over rows.
    monotone_constraints: ForestTrainer's, as FEATURES_COUNT signs or as a dict by FEATURE_NAMES
    (feature_engineering.ratio_constraints() constrains the 17 similarity ratios upwards), handed to fit_device.
    permutation_repeats: 0, or the n_repeats of ForestModel.permutation_importance_device, run on the evaluation
    matrix where it lies in HBM after the error matrix, with seed permutation_seed and the fit's beta: the result's
    `permutation_importance`, timed as `timings["permutation"]`.  It needs an evaluation set.
    bootstrap_repeats: 0, or the n_boot of bootstrap.compare_models_device, run on the evaluation matrix where it lies
    in HBM with seed bootstrap_seed, the fit's beta and the evaluation rows grouped by the train title they were
    sampled for (tuning.row_groups): the result's `error_bootstrap`, timed as `timings["bootstrap"]`.  With init_model
    it holds two sets, "model" and "init_model", and difference("model", "init_model") says whether the continued
    model's gain exceeds what another evaluation sample would give.  It needs an evaluation set.
    calibrate: True fits what the model's probability means on the evaluation matrix where it lies in HBM
    (ForestModel.calibrate_device) and bins it before and after in reliability_bins bins: the result's `calibrator`,
    `reliability` and `calibrated_reliability`, timed as `timings["calibration"]`.  It needs an evaluation set.  That
    set also chose best_iteration, and the calibrated report is read on the rows the map was fitted to, so it is mildly
    optimistic: a held-out set through ForestModel.calibrate is the honest one.  False makes exactly the calls made
    without it.
    misspelling_profile: FeatureEngineering's: None, a MisspellingProfile after which the generated rows are misspelled,
    or "fit" to learn it from this call's own labelled train pairs first; the result's `misspelling_profile` is the
    profile that was used (None without one)."""
    from .feature_engineering import FEATURES_COUNT, FEATURE_NAMES
    from .training_set import FeatureEngineering, kind_weights as weights_of_kinds, validate_kind_weights
    started = time.perf_counter()
    unknown = set(fit_parameters) - set(inspect.signature(validate_parameters).parameters)
    if unknown:
        raise ValueError(f"unknown fit parameters {sorted(unknown)}")
    validate_parameters(**fit_parameters)
    if init_model is not None:
        validate_init_model(init_model, FEATURES_COUNT, device)
    if kind_weights is not None:
        validate_kind_weights(kind_weights)
    if monotone_constraints is not None:
        monotone_constraints = validate_monotone_constraints(monotone_constraints, FEATURES_COUNT, FEATURE_NAMES)
    permutation_repeats = _positive_int("permutation_repeats", permutation_repeats, 0, (1 << 16) - 1)
    permutation_seed = _positive_int("permutation_seed", permutation_seed, 0, (1 << 63) - 1)
    bootstrap_repeats = _positive_int("bootstrap_repeats", bootstrap_repeats, 0, 1 << 16)
    bootstrap_seed = _positive_int("bootstrap_seed", bootstrap_seed, 0, (1 << 63) - 1)
    if not isinstance(calibrate, (bool, np.bool_)):
        raise ValueError(f"calibrate must be True or False, not {calibrate!r}")
    if calibrate:
        from .calibration import calibrate_rows_device, validate_calibration
        reliability_bins = validate_calibration(n_bins=reliability_bins)["n_bins"]
    fe = FeatureEngineering(truth_titles, truth_title_ids, train_titles, train_title_ids, top_n=top_n,
                            sample_n=sample_n, seed=seed, device=device, transform=transform,
                            evaluation_fractions=evaluation_fractions, build_index=build_index,
                            misspelling_profile=misspelling_profile)
    if permutation_repeats and not any(fe.evaluation_fractions.values()):
        raise ValueError("permutation_repeats needs an evaluation set, and every evaluation fraction is 0")
    if bootstrap_repeats and not any(fe.evaluation_fractions.values()):
        raise ValueError("bootstrap_repeats needs an evaluation set, and every evaluation fraction is 0")
    if calibrate and not any(fe.evaluation_fractions.values()):
        raise ValueError("calibrate needs an evaluation set, and every evaluation fraction is 0")
    sets = fe.generate_device_data_sets()
    timings = dict(fe.timings)
    if permutation_repeats and sets.n_evaluation == 0:
        sets.free()
        raise ValueError("permutation_repeats needs an evaluation set, and no row was drawn into it")
    if bootstrap_repeats and sets.n_evaluation == 0:
        sets.free()
        raise ValueError("bootstrap_repeats needs an evaluation set, and no row was drawn into it")
    if calibrate and sets.n_evaluation == 0:
        sets.free()
        raise ValueError("calibrate needs an evaluation set, and no row was drawn into it")
    trainer = ForestTrainer(device)
    mark = time.perf_counter()
    has_eval = sets.n_evaluation > 0
    weighted = {} if kind_weights is None else dict(sample_weight=weights_of_kinds(fe.rows, kind_weights))
    try:
        model = trainer.fit_device(sets.train, sets.n_train, sets.train_target, sets.evaluation if has_eval else None,
                                   sets.n_evaluation, sets.evaluation_target if has_eval else None,
                                   init_model=init_model, monotone_constraints=monotone_constraints, **weighted,
                                   **fit_parameters)
    except ValueError:              # weights the rows of this training set cannot carry: free what the call holds
        sets.free()
        raise
    fit_ms = (time.perf_counter() - mark) * 1000.0
    timings["cuts"], timings["bin"] = trainer.timings["cuts"], trainer.timings["bin"]
    timings["boost"] = fit_ms - timings["cuts"] - timings["bin"]
    mark = time.perf_counter()
    error_matrix = None
    if has_eval:
        d_probabilities = _lib.DeviceArray((sets.n_evaluation,), np.float32, device)
        model.predict_device(sets.evaluation, sets.n_evaluation, None, d_probabilities)
        error_matrix = _error_matrix(d_probabilities.to_host(), sets.evaluation_target,
                                     PREDICTION_PROBABILITY_THRESHOLD)
        d_probabilities.free()
    timings["evaluate"] = (time.perf_counter() - mark) * 1000.0
    permutation_importance = None
    if permutation_repeats:
        mark = time.perf_counter()
        d_target = _lib.DeviceArray.from_host(np.ascontiguousarray(sets.evaluation_target, dtype=np.float32), device)
        try:
            permutation_importance = model.permutation_importance_device(
                sets.evaluation, sets.n_evaluation, d_target, n_repeats=permutation_repeats, seed=permutation_seed,
                beta=validate_parameters(**fit_parameters)["beta"])
        finally:
            d_target.free()
        timings["permutation"] = (time.perf_counter() - mark) * 1000.0
    error_bootstrap = None
    if bootstrap_repeats:
        from .bootstrap import compare_models_device
        from .tuning import row_groups
        mark = time.perf_counter()
        d_target = _lib.DeviceArray.from_host(np.ascontiguousarray(sets.evaluation_target, dtype=np.float32), device)
        compared = [model] if init_model is None else [model, init_model]
        try:
            error_bootstrap = compare_models_device(
                compared, sets.evaluation, sets.n_evaluation, d_target,
                groups=row_groups(fe.rows)[fe.rows["evaluation"].to_numpy()], n_boot=bootstrap_repeats,
                seed=bootstrap_seed, threshold=PREDICTION_PROBABILITY_THRESHOLD,
                beta=validate_parameters(**fit_parameters)["beta"], names=("model", "init_model")[:len(compared)])
        finally:
            d_target.free()
        timings["bootstrap"] = (time.perf_counter() - mark) * 1000.0
    calibration = (None, None, None)
    if calibrate:
        mark = time.perf_counter()
        d_target = _lib.DeviceArray.from_host(np.ascontiguousarray(sets.evaluation_target, dtype=np.float32), device)
        try:
            calibration = calibrate_rows_device(model, sets.evaluation, sets.n_evaluation, d_target, reliability_bins)
        finally:
            d_target.free()
        timings["calibration"] = (time.perf_counter() - mark) * 1000.0
    if cover:
        mark = time.perf_counter()
        try:
            model.fit_cover_device(sets.train, sets.n_train)
        except ValueError:          # a node no training row reached: free what the call holds before it leaves
            trainer.close()
            sets.free()
            raise
        timings["cover"] = (time.perf_counter() - mark) * 1000.0
    best_iteration, history, initial_error = trainer.best_iteration, list(trainer.history), trainer.initial_error
    metrics_history = {key: list(values) for key, values in trainer.metrics_history.items()} \
        if trainer.eval_metrics else None
    trainer.close()
    sets.free()
    timings["total"] = (time.perf_counter() - started) * 1000.0
    return TrainModelResult(model, model.feature_importance(), error_matrix, best_iteration, history, fe.rows, timings,
                            metrics_history=metrics_history, initial_error=initial_error,
                            permutation_importance=permutation_importance, error_bootstrap=error_bootstrap,
                            calibrator=calibration[0], reliability=calibration[1],
                            calibrated_reliability=calibration[2], misspelling_profile=fe.misspelling_profile)
