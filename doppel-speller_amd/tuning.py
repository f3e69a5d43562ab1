"""Cross-validation and parameter search for the match model ("Cross-validation and tuning").

ForestTrainerBatch grows many boosters over ONE binned matrix on the GPU (csrc/ds_train_batch.hip, C ABI
ds_trainer_batch_*): every model has its own parameters and its own held-out fold, and one round launches each kernel
once for all of them.  cross_validate runs K folds x P parameter sets on it with xgb.cv's rule (the per-round sum of the
folds' integer errors, the first minimum, early stopping on that sum) and refits the chosen set on all rows;
tune_model_parameters does so from raw titles with the feature matrix never leaving HBM.
"""
import ctypes
import inspect
import itertools
import time

import numpy as np

from . import _lib
from .train import (METRIC_NAMES, SAMPLING_NAMES, FirstMinimum, _call, _device_columns, _device_labels,
                    _matrix_and_labels, _positive_int, _samples, _TrainerHandle, auc_numerator, compute_cuts,
                    compute_cuts_device, heap_tree, metric_values, validate_init_model, validate_metrics,
                    validate_monotone_constraints, validate_parameters, validate_sample_weight)

MODELS_MAX = 256          # ds_train_batch.hip kBatchModelsMax
FOLDS_MAX = 255           # ds_train_batch.hip kBatchFoldsMax
PARAMETER_NAMES = ("max_depth", "eta", "min_child_weight", "reg_lambda", "beta")
# the subsampling parameters (train.SAMPLING_NAMES): a parameter set carries them only when some set of its list names one
_DEFAULTS = {name: inspect.signature(validate_parameters).parameters[name].default
             for name in PARAMETER_NAMES + SAMPLING_NAMES}


def _names_sampling(sets):
    return any(isinstance(one, dict) and name in one for one in sets for name in SAMPLING_NAMES)


def _parameter_set(parameters, what="parameters", sampling=None):
    """One dict of the five booster parameters, defaults filled in, checked by validate_parameters; with `sampling`
    (default: when the dict names one of SAMPLING_NAMES) the four subsampling parameters follow them."""
    known = PARAMETER_NAMES + SAMPLING_NAMES
    if not isinstance(parameters, dict):
        raise ValueError(f"{what} must be a dict of {known}, not {parameters!r}")
    unknown = set(parameters) - set(known)
    if unknown:
        raise ValueError(f"unknown {what} {sorted(unknown)}; known: {list(known)}")
    if sampling is None:
        sampling = _names_sampling([parameters])
    checked = validate_parameters(**dict(_DEFAULTS, **parameters))
    return {name: checked[name] for name in (known if sampling else PARAMETER_NAMES)}


def _parameter_sets(parameters):
    sets = [parameters] if isinstance(parameters, dict) else list(parameters) if parameters is not None else []
    if not sets:
        raise ValueError("parameters must be a parameter dict or a non-empty list of them")
    sampling = _names_sampling(sets)
    sets = [_parameter_set(one, sampling=sampling) for one in sets]
    keys = [tuple(one.values()) for one in sets]
    if len(set(keys)) != len(keys):
        raise ValueError("parameters holds the same parameter set twice")
    return sets


def parameter_grid(**lists):
    """The Cartesian product of max_depth, eta, min_child_weight, reg_lambda and beta (a scalar counts as a list of
    one, a parameter left out takes its default) as a list of parameter dicts.  The order is fixed: the parameters
    vary in the order just named, the LAST-named one fastest (itertools.product).  Every set is checked by
    validate_parameters; a value given twice, which would make two equal sets, is refused.
    When one of subsample, colsample_bytree, colsample_bylevel and sample_seed is given, the four join the product
    after beta, in that order, and every dict carries all nine; otherwise the dicts have the five keys alone."""
    names = PARAMETER_NAMES + SAMPLING_NAMES
    unknown = set(lists) - set(names)
    if unknown:
        raise ValueError(f"unknown parameters {sorted(unknown)}; known: {list(names)}")
    if not _names_sampling([lists]):
        names = PARAMETER_NAMES
    axes = []
    for name in names:
        values = lists.get(name, _DEFAULTS[name])
        values = list(values) if isinstance(values, (list, tuple, np.ndarray)) else [values]
        if not values:
            raise ValueError(f"{name} has no values")
        axes.append(values)
    return _parameter_sets([dict(zip(names, combination)) for combination in itertools.product(*axes)])


def fold_assignment(groups, n_folds, seed=0, n=None):
    """uint8[n]: the fold of every row.  The distinct group values in ascending order are permuted by
    np.random.default_rng(seed).permutation; the group at position i of the permuted order gets fold i % n_folds, so
    rows of one group share a fold, the folds' sizes in groups differ by at most one, and the result depends on the
    values of `groups` alone, not on the order of the rows.  groups=None: every one of the n rows is its own group."""
    n_folds = _positive_int("n_folds", n_folds, 2, FOLDS_MAX)
    seed = _positive_int("seed", seed, 0)
    if groups is None:
        if n is None:
            raise ValueError("without groups the number of rows is needed: fold_assignment(None, n_folds, seed, n=rows)")
        n_groups = _positive_int("n", n, 1)
        inverse = np.arange(n_groups)
    else:
        groups = np.asarray(groups)
        if groups.ndim != 1 or groups.shape[0] < 1:
            raise ValueError(f"groups must be a non-empty 1-D array, not shape {groups.shape}")
        if n is not None and groups.shape[0] != n:
            raise ValueError(f"{n} rows but {groups.shape[0]} groups")
        distinct, inverse = np.unique(groups, return_inverse=True)
        n_groups = distinct.shape[0]
    if n_folds > n_groups:
        raise ValueError(f"n_folds = {n_folds} exceeds the {n_groups} groups")
    fold_of_group = np.empty(n_groups, np.uint8)
    fold_of_group[np.random.default_rng(seed).permutation(n_groups)] = np.arange(n_groups) % n_folds
    return fold_of_group[inverse.reshape(-1)]


SELECT_BY = ("error",) + METRIC_NAMES


def validate_selection(metrics=(), select_by="error"):
    """cross_validate's `metrics` and `select_by` -> (metrics in METRIC_NAMES' order, select_by)."""
    metrics = validate_metrics(metrics, "metrics")
    if not isinstance(select_by, str) or select_by not in SELECT_BY:
        raise ValueError(f"select_by must be one of {SELECT_BY}, not {select_by!r}")
    if select_by != "error" and select_by not in metrics:
        raise ValueError(f"select_by = {select_by!r} needs that metric: metrics = {metrics!r} does not request it")
    return metrics, select_by


def pooled_counts(fold_counts):
    """The out-of-fold integers of one round: the sums over the folds of (concordant, ties, positives * negatives,
    logloss_sum, rows) from each fold's (concordant, ties, positives, negatives, logloss_sum, rows); an entry whose
    metric was not requested (-1 in a fold) is -1."""
    folds = [tuple(int(v) for v in one) for one in fold_counts]
    auc = all(one[0] >= 0 for one in folds)
    logloss = all(one[4] >= 0 for one in folds)
    return (sum(one[0] for one in folds) if auc else -1, sum(one[1] for one in folds) if auc else -1,
            sum(one[2] * one[3] for one in folds) if auc else -1,
            sum(one[4] for one in folds) if logloss else -1, sum(one[5] for one in folds) if logloss else -1)


def pooled_values(pooled):
    """{auc, logloss} of pooled_counts: auc = sum(2 c + t) / (2 sum(P N)), logloss = sum / 2^20 / rows: ratios of
    integer sums, the same whatever the order of the folds."""
    out = {}
    if pooled[0] >= 0:
        out["auc"] = (2 * pooled[0] + pooled[1]) / (2 * pooled[2]) if pooled[2] > 0 else float("nan")
    if pooled[3] >= 0:
        out["logloss"] = pooled[3] / float(1 << 20) / pooled[4] if pooled[4] > 0 else float("nan")
    return out


def _selection_score(select_by, errors, fold_counts):
    """The integer that a round is judged by, smaller = better: the summed error; minus the pooled AUC numerator
    sum(2 c + t); the pooled log-loss sum.  The denominators (pairs, rows) are those of the folds and the labels, the
    same for every parameter set and round, so the numerators order the values exactly."""
    if select_by == "error":
        return int(sum(int(e) for e in errors))
    pooled = pooled_counts(fold_counts)
    if pooled[0 if select_by == "auc" else 3] < 0:
        raise ValueError(f"select_by = {select_by!r}, but the metric counts do not hold that metric")
    return -(2 * pooled[0] + pooled[1]) if select_by == "auc" else pooled[3]


def _replay(curve, early_stopping_rounds):
    """(best_iteration, error, rounds) of one summed curve under the stepping rule: the first minimum; the set stops
    after the first round with round - best >= early_stopping_rounds (None: never), later entries are not looked at."""
    rule = FirstMinimum(early_stopping_rounds)
    rounds = next((round_ + 1 for round_, error in enumerate(curve) if rule.see(round_, error)), len(curve))
    return rule.best, int(rule.value), rounds


def select_parameters(histories, early_stopping_rounds=None, select_by="error", metric_counts=None):
    """xgb.cv's choice, on the host.  histories[p][k] = the held-out error of fold k after every round of parameter set
    p (the K curves of a set have one length; sets may differ).  Per set the summed curve is the per-round sum of its
    folds' errors -- the out-of-fold error over the whole matrix, an integer -- best_iteration its first minimum and
    error that minimum, looking no further than the round at which early_stopping_rounds would have stopped the set.
    The chosen set has the lowest error; a tie goes to the smaller best_iteration, then to the earlier set.
    Returns dict(chosen, best_iteration[p], error[p], rounds[p], history[p]).

    metric_counts[p][k][r] = the six integers (train.COUNT_NAMES) of fold k's held-out rows after round r.  With them
    the result gains metrics_history[p] = {"auc": [...], "logloss": [...]}, the pooled out-of-fold value of every round
    looked at (pooled_values).  select_by = "auc" (maximise) or "logloss" (minimise) runs the same rule -- first best
    round, early stopping, ties to the smaller best_iteration, then the earlier set -- on that metric's pooled curve
    instead of the error's, comparing its integer numerators (_selection_score); error[p] and history[p] stay the
    summed error, error[p] taken at the best_iteration so chosen, and score[p] is the numerator there."""
    if early_stopping_rounds is not None:
        early_stopping_rounds = _positive_int("early_stopping_rounds", early_stopping_rounds)
    if not isinstance(select_by, str) or select_by not in SELECT_BY:
        raise ValueError(f"select_by must be one of {SELECT_BY}, not {select_by!r}")
    if select_by != "error" and metric_counts is None:
        raise ValueError(f"select_by = {select_by!r} needs that metric: no metric was requested")
    if len(histories) == 0:
        raise ValueError("histories is empty")
    if metric_counts is not None and len(metric_counts) != len(histories):
        raise ValueError(f"{len(histories)} parameter sets but metric counts of {len(metric_counts)}")
    out = dict(best_iteration=[], error=[], rounds=[], history=[])
    if metric_counts is not None:
        out["metrics_history"] = []
    if select_by != "error":
        out["score"] = []
    for p, folds in enumerate(histories):
        lengths = {len(curve) for curve in folds}
        if len(folds) == 0 or len(lengths) != 1 or 0 in lengths:
            raise ValueError(f"parameter set {p}: the folds' curves must be non-empty and of one length")
        length = lengths.pop()
        summed = [int(sum(int(curve[r]) for curve in folds)) for r in range(length)]
        if metric_counts is not None and (len(metric_counts[p]) != len(folds) or
                                          {len(curve) for curve in metric_counts[p]} != {length}):
            raise ValueError(f"parameter set {p}: the metric counts must have the shape of the folds' curves")
        if select_by == "error":
            best, error, rounds = _replay(summed, early_stopping_rounds)
        else:
            scores = [_selection_score(select_by, None, [curve[r] for curve in metric_counts[p]])
                      for r in range(length)]
            best, score, rounds = _replay(scores, early_stopping_rounds)
            error = summed[best]
            out["score"].append(score)
        out["best_iteration"].append(best)
        out["error"].append(error)
        out["rounds"].append(rounds)
        out["history"].append(summed[:rounds])
        if metric_counts is not None:
            values = [pooled_values(pooled_counts([curve[r] for curve in metric_counts[p]])) for r in range(rounds)]
            out["metrics_history"].append({name: [one[name] for one in values] for name in (values[0] if values else ())})
    judged = out["error"] if select_by == "error" else out["score"]
    out["chosen"] = min(range(len(histories)), key=lambda p: (judged[p], out["best_iteration"][p], p))
    return out


def validate_models(models, n_folds):
    """The model list of ForestTrainerBatch.begin -> (params float64[M, 5], held_out int32[M], parameter dicts)."""
    models = list(models) if models is not None else []
    if not 1 <= len(models) <= MODELS_MAX:
        raise ValueError(f"a batch takes 1 to {MODELS_MAX} models, not {len(models)}")
    sets, held = [], []
    sampling = _names_sampling(models)      # some model names a subsampling parameter: every set carries the four
    for m, model in enumerate(models):
        if not isinstance(model, dict):
            raise ValueError(f"model {m} must be a dict, not {model!r}")
        sets.append(_parameter_set({k: v for k, v in model.items() if k != "held_out"}, f"parameters of model {m}",
                                   sampling))
        held.append(_positive_int(f"held_out of model {m}", model.get("held_out", -1), -1, n_folds - 1))
    params = np.array([[one[name] for name in PARAMETER_NAMES] for one in sets], np.float64)
    return np.ascontiguousarray(params), np.array(held, np.int32), sets


def validate_batch_weight(sample_weight, n, fold, held_out, sets):
    """The checks of a batch's `sample_weight` (no library needed) -> float32[n]: validate_sample_weight over all rows
    with the largest beta among the models, and per model a total above 0 over ITS training rows (those outside its
    held-out fold); the first model without one is named."""
    weights = validate_sample_weight(sample_weight, n, max(one["beta"] for one in sets))
    positive = np.bincount(fold[weights > 0], minlength=FOLDS_MAX + 1) > 0      # the folds that weigh something
    for m, held in enumerate(held_out):
        if not positive[np.arange(positive.shape[0]) != held].any():
            raise ValueError(f"model {m}: the total sample weight of its training rows (outside fold {int(held)}) is 0")
    return weights


def _validate_fold(fold, n):
    fold = np.asarray(fold)
    if fold.ndim != 1 or fold.shape[0] != n:
        raise ValueError(f"{n} rows but {fold.reshape(-1).shape[0]} fold entries")
    if not np.issubdtype(fold.dtype, np.integer) or fold.min() < 0 or fold.max() >= FOLDS_MAX:
        raise ValueError(f"fold must hold integers in [0, {FOLDS_MAX})")
    return np.ascontiguousarray(fold, dtype=np.uint8), int(fold.max()) + 1


def batch_bytes(n, n_features, n_models, max_depth):
    """ds_trainer_batch_bytes: the HBM a batch of n_models models over n x n_features needs (a host matrix adds its
    staged copy, 4 * n * n_features)."""
    return int(_lib.lib().ds_trainer_batch_bytes(n, n_features, n_models, max_depth))


def batch_metrics_bytes(n, n_models, n_folds):
    """ds_trainer_batch_metrics_bytes: the HBM that per-round metrics add to a batch with folds of equal size."""
    return int(_lib.lib().ds_trainer_batch_metrics_bytes(n, n_models, n_folds))


def batch_option(name, value):
    """ds_trainer_batch_option, for tests: batch_option("max_blocks", b) caps the row grids (0: default)."""
    _lib.set_option("ds_trainer_batch_option", name, value)


class ForestTrainerBatch(_TrainerHandle):
    """Many ForestTrainers over one binned matrix, stepped together.

        batch = ForestTrainerBatch().begin(features, target, fold, models)
        errors = batch.step()            # one round of every model; errors[m] = held-out error, None without a fold

    models: dicts {max_depth, eta, min_child_weight, reg_lambda, beta, held_out} and, optionally, {subsample,
    colsample_bytree, colsample_bylevel, sample_seed} (every model its own); row r trains in model m iff
    fold[r] != held_out (-1, the default: every row trains).  The cuts are those of the WHOLE matrix, so a model's trees
    are ForestTrainer's on its training rows with those cuts.  step(active) touches only the models with active[m] true.
    trees[m], history[m] (errors; None entries without a fold), model(m, n_trees), margins(m) (all rows),
    probabilities(m), gradients(m), bins(), last_heap[m] as ForestTrainer's.

    begin(..., metrics=("auc", "logloss")) also computes, in every step and on the device, the metrics of each active
    model over the rows of its HELD-OUT fold: metric_counts[m] gains the round's (concordant, ties, positives, negatives,
    logloss_sum, rows) and metrics_history[m][name] its value (-1s and None for a model without a fold).

    begin(..., init_model=<ForestModel>) starts EVERY model from that model ("Continuing from a
    model"): the forest is evaluated once per row of the raw matrix on the device, `initial_errors[m]` is its error on
    model m's held-out rows (None without a fold), trees[m] and history[m] hold the new rounds, model(m, n) the init
    trees followed by the first n new ones, and model m stays ForestTrainer(init_model=...)'s on its training rows.

    begin(..., sample_weight=<array of n numbers>) weighs the rows in every model's objective (DESIGN.md section 9,
    "Sample weights"): ONE array over all rows, like the labels; model m is ForestTrainer(sample_weight=...)'s on its
    training rows with their weights, and a held-out row trains nothing whatever its weight.  Every model's training
    rows need a total weight above 0 (validate_batch_weight names the model that has none).  The held-out errors and
    the metrics stay counts over rows.

    begin(..., monotone_constraints=<n_features signs>) constrains every model alike ("Monotone
    constraints"): ONE vector for the batch, and model m is ForestTrainer(monotone_constraints=...)'s on its training
    rows.  None or all zeros makes exactly the calls of a batch that knows no constraints."""
    ENTRIES, READS = "ds_trainer_batch", ("margins", "probabilities", "gradients", "bins")

    def __init__(self, device=0):
        self.device = device
        self.handle = None
        self.trees, self.history, self.last_heap = [], [], []
        self.metrics, self.metrics_history, self.metric_counts = (), [], []
        self.init_model, self.initial_errors = None, []
        self.sample_weight = None
        self.monotone_constraints = None
        self.timings = {}

    def begin(self, features, target, fold, models, max_bin=256, cuts=None, metrics=(), init_model=None,
              sample_weight=None, monotone_constraints=None):
        features, target = _matrix_and_labels(features, target, "training")
        return self._begin(features, False, features.shape[0], features.shape[1], target, fold, models, max_bin, cuts,
                           metrics, init_model, sample_weight, monotone_constraints)

    def begin_device(self, d_features, n, target, fold, models, n_features=None, max_bin=256, cuts=None, metrics=(),
                     init_model=None, sample_weight=None, monotone_constraints=None):
        """begin for a contiguous float32[n, n_features] matrix that lies complete in HBM (a DeviceArray, or an address
        with n_features given).  It is read where it lies, never copied to the host, and not kept."""
        n_features = _device_columns(d_features, n_features)
        n, target = _device_labels(n, target, "training")
        if isinstance(d_features, _lib.DeviceArray) and n > d_features.shape[0]:
            raise ValueError(f"{n} training rows exceed the device matrix's {d_features.shape[0]}")
        return self._begin(d_features, True, n, n_features, target, fold, models, max_bin, cuts, metrics, init_model,
                           sample_weight, monotone_constraints)

    def _begin(self, features, in_hbm, n, n_features, target, fold, models, max_bin, cuts, metrics=(), init_model=None,
               sample_weight=None, monotone_constraints=None):
        metrics = validate_metrics(metrics, "metrics")
        if init_model is not None:
            validate_init_model(init_model, n_features, self.device)
        fold, n_folds = _validate_fold(fold, n)
        params, held_out, sets = validate_models(models, FOLDS_MAX)
        if held_out.max() >= n_folds:
            raise ValueError(f"held_out = {int(held_out.max())} but fold holds only 0 .. {n_folds - 1}")
        max_bin = _positive_int("max_bin", max_bin, 2, 256)
        if sample_weight is not None:
            sample_weight = validate_batch_weight(sample_weight, n, fold, held_out, sets)
        if monotone_constraints is not None:
            monotone_constraints = validate_monotone_constraints(monotone_constraints, n_features)
        self.close()
        self.sample_weight = sample_weight
        self.monotone_constraints = monotone_constraints
        self.timings = {}
        mark = time.perf_counter()
        if cuts is None:
            cuts = compute_cuts_device(features, n, max_bin, n_features, self.device) if in_hbm else \
                compute_cuts(features, max_bin)
        self.cuts, self.cut_offsets = cuts
        self.timings["cuts"] = (time.perf_counter() - mark) * 1000.0
        self.n, self.n_features, self.n_models, self.n_folds = n, n_features, len(sets), n_folds
        self.parameters, self.held_out = sets, held_out
        self.max_depth = int(params[:, 0].max())
        self.trees = [[] for _ in sets]
        self.history = [[] for _ in sets]
        self.last_heap = [None] * len(sets)
        mark = time.perf_counter()
        handle = ctypes.c_void_p()
        _call("ds_trainer_batch_create", in_hbm, _lib.pointer(features), n, n_features, _lib.pointer(self.cuts),
              _lib.pointer(self.cut_offsets), _lib.pointer(target), _lib.pointer(fold), n_folds, self.n_models,
              _lib.pointer(params), _lib.pointer(held_out), self.device, ctypes.byref(handle))
        self.handle = handle
        if sample_weight is not None:
            _lib.check(_lib.lib().ds_trainer_batch_set_weights(self.handle, _lib.pointer(sample_weight)),
                       "ds_trainer_batch_set_weights")
        if monotone_constraints is not None and monotone_constraints.any():   # none or all zeros: nothing to set
            _lib.check(_lib.lib().ds_trainer_batch_set_monotone(self.handle, _lib.pointer(monotone_constraints)),
                       "ds_trainer_batch_set_monotone")
        if any(_samples(one) for one in sets):
            fractions = np.array([[one[name] for name in SAMPLING_NAMES[:3]] for one in sets], np.float64)
            seeds = np.array([one["sample_seed"] for one in sets], np.uint64)
            _lib.check(_lib.lib().ds_trainer_batch_set_sampling(self.handle, _lib.pointer(fractions),
                                                                _lib.pointer(seeds)), "ds_trainer_batch_set_sampling")
        self.init_model, self.initial_errors = init_model, [None] * len(sets)
        if init_model is not None:
            errors = np.full(self.n_models, -1, np.int64)
            _call("ds_trainer_batch_seed", in_hbm, self.handle, init_model.handle, _lib.pointer(features),
                  _lib.pointer(errors), *((None,) if in_hbm else ()))
            self.initial_errors = [int(errors[m]) if held_out[m] >= 0 else None for m in range(self.n_models)]
        self.metrics = metrics
        self.metrics_history = [{name: [] for name in metrics} for _ in sets]
        self.metric_counts = [[] for _ in sets]
        self._set_metrics(metrics, self.n_models)
        self.timings["bin"] = (time.perf_counter() - mark) * 1000.0
        slots = (2 << self.max_depth) - 1          # the heaps of every model have the largest max_depth's slots
        self._info = np.zeros((self.n_models, slots, 4), np.int32)
        self._leaf = np.zeros((self.n_models, slots), np.float32)
        self._errors = np.zeros(self.n_models, np.int64)
        return self

    def step(self, active=None):
        """One round of the active models (default: all).  Returns a list with the held-out error of every model that
        stepped and has a held-out fold, None for the others."""
        if not self.handle:
            raise RuntimeError("ForestTrainerBatch.step before begin")
        if active is None:
            mask = np.ones(self.n_models, np.uint8)
        else:
            mask = np.ascontiguousarray(np.asarray(active).astype(bool), dtype=np.uint8)
            if mask.shape != (self.n_models,):
                raise ValueError(f"active must have {self.n_models} entries, not shape {mask.shape}")
        _lib.check(_lib.lib().ds_trainer_batch_step(self.handle, _lib.pointer(mask), _lib.pointer(self._info),
                                                    _lib.pointer(self._leaf), _lib.pointer(self._errors)),
                   "ds_trainer_batch_step")
        if self.metrics:
            _lib.check(_lib.lib().ds_trainer_batch_metrics(self.handle, _lib.pointer(self._metric_counts)),
                       "ds_trainer_batch_metrics")
        out = [None] * self.n_models
        for m in np.nonzero(mask)[0]:
            if self.metrics:
                held = self.held_out[m] >= 0
                self.metric_counts[m].append(tuple(int(v) for v in self._metric_counts[m]))
                values = metric_values(self._metric_counts[m], self.metrics) if held else {}
                for name in self.metrics:
                    self.metrics_history[m][name].append(values.get(name))
            self.last_heap[m] = (self._info[m].copy(), self._leaf[m].copy())
            self.trees[m].append(heap_tree(self._info[m], self._leaf[m], self.cuts, self.cut_offsets))
            out[m] = int(self._errors[m]) if self.held_out[m] >= 0 else None
            self.history[m].append(out[m])
        return out

    def model(self, m, n_trees=None):
        """ForestModel of the first n_trees trees of model m grown here (default: all so far), after the init model's
        if there is one."""
        return self._model(self.trees[m], n_trees)

    def margins(self, m):
        """Model m's margins of ALL rows after its trees so far (float32[n])."""
        return self._read(m, margins=(self.n, np.float32))["margins"]

    def probabilities(self, m):
        return self._read(m, probabilities=(self.n, np.float32))["probabilities"]

    def gradients(self, m):
        """int64[n, 2] of model m's last step; (0, 0) in its held-out rows."""
        return self._read(m, gradients=((self.n, 2), np.int64))["gradients"]

    def bins(self):
        return self._read(0, bins=((self.n_features, self.n), np.uint8))["bins"]


class CrossValidation:
    """What cross_validate returns: `results` (DataFrame, one line per parameter set in the given order: the five
    parameters -- then the four subsampling ones when a set names one --, best_iteration, error, rounds, fold_errors at
    the best round), `history[p]` (the summed curve),
    `fold_history[p][k]`, `parameters` (the sets), `chosen` (the index of the best set), `best_parameters`,
    `best_iteration`, `folds` (uint8[n]), `timings` (ms: cuts, bin, boost, refit, total) and, with refit, `model`.
    With metrics: `metrics_history[p]` ({"auc": [...], "logloss": [...]}: per round the pooled out-of-fold value of set
    p), `fold_metric_counts[p][k]` (per round the six integers of fold k), `select_by`, and the columns `auc` and/or
    `logloss` of `results` at best_iteration.
    With init_model: `initial_errors[p]`, the pooled out-of-fold error of the init model under set p's folds (the same
    number for every set: the baseline that "did continuing help" is judged against) and the column `initial_error`;
    rounds, curves and best_iteration count the NEW rounds, and `model` has the init trees before them.
    tune_model_parameters adds `rows` and `feature_importance`."""

    def __init__(self, **fields):
        self.model = self.rows = self.feature_importance = None
        self.__dict__.update(fields)


def validate_cross_validation(parameters, n_folds=5, seed=0, num_boost_round=1000, early_stopping_rounds=50,
                              max_bin=256, models_per_batch=None, metrics=(), select_by="error"):
    """cross_validate's checks of everything but the data (no library needed) -> (parameter sets, sets per batch)."""
    sets = _parameter_sets(parameters)
    validate_selection(metrics, select_by)
    n_folds = _positive_int("n_folds", n_folds, 2, FOLDS_MAX)
    _positive_int("seed", seed, 0)
    validate_parameters(num_boost_round=num_boost_round, early_stopping_rounds=early_stopping_rounds, max_bin=max_bin)
    if models_per_batch is not None:
        models_per_batch = _positive_int("models_per_batch", models_per_batch, 1, MODELS_MAX)
        if models_per_batch < n_folds:
            raise ValueError(f"models_per_batch = {models_per_batch} is below n_folds = {n_folds}: a batch holds whole "
                             "parameter sets")
        return sets, models_per_batch // n_folds
    return sets, None


def _sets_per_batch(n, n_features, in_hbm, sets, n_folds, device, metrics=(), weighted=False):
    """Whole parameter sets (K models each) per batch: what 80 % of the free HBM holds, 256 models at most.  With
    metrics their scratch (batch_metrics_bytes) comes off the budget, with sample weights their 4 n bytes."""
    free, total = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(_lib.lib().ds_device_memory(device, ctypes.byref(free), ctypes.byref(total)), "ds_device_memory")
    budget = int(free.value * 0.8) - (0 if in_hbm else 4 * n * n_features) - (4 * n if weighted else 0)
    depth = max(one["max_depth"] for one in sets)
    count = max(1, min(len(sets), MODELS_MAX // n_folds))
    extra = (lambda models: batch_metrics_bytes(n, models, n_folds)) if metrics else (lambda models: 0)
    while count > 1 and batch_bytes(n, n_features, count * n_folds, depth) + extra(count * n_folds) > budget:
        count -= 1
    return count


def cross_validate(features, target, parameters, n_folds=5, groups=None, seed=0, num_boost_round=1000,
                   early_stopping_rounds=50, max_bin=256, refit=True, device=0, models_per_batch=None, metrics=(),
                   select_by="error", init_model=None, sample_weight=None, monotone_constraints=None):
    """K-fold cross-validation of one parameter set or a list of them (parameter_grid) on the GPU -> CrossValidation.

    features: a host matrix, or a DeviceArray float32[>= n, n_features] in HBM of which the first len(target) rows
    count (never copied to the host).  The folds come from fold_assignment(groups, n_folds, seed).  Every set runs
    n_folds models, model k holding fold k out, all stepped together in batches of whole sets.  A set is stepped until
    round - best >= early_stopping_rounds on its SUMMED curve or until num_boost_round; then its models go inactive
    while other sets continue.  models_per_batch=None sizes the batches from the free HBM; the result does not depend
    on it.  The cuts are computed once, the bins once per batch.  A set with subsampling parameters uses its
    sample_seed in every fold.  refit: the chosen set is trained on ALL rows for
    best_iteration + 1 rounds; with the whole matrix's cuts that is ForestTrainer().fit(features, target,
    num_boost_round=best_iteration + 1, **best_parameters), bit for bit.

    metrics=("auc", "logloss"): every step also computes these over each model's held-out rows, on the device (DESIGN.md
    section 9, "Metrics"); the result gains metrics_history[p] (the pooled out-of-fold value per round: auc =
    sum_k (2 c_k + t_k) / (2 sum_k P_k N_k), logloss = sum_k sum_k / 2^20 / sum_k rows_k) and the columns `auc` /
    `logloss` of `results`.  select_by = "auc" (maximise) or "logloss" (minimise) steps, stops and chooses on that curve
    instead of the error's, by its integer numerators; "error" (the default) is the rule above whatever the metrics.

    init_model: every fold of every set starts from that ForestModel ("Continuing from a model").
    Rounds, curves and best_iteration count the new rounds; `initial_errors` gives the init model's pooled out-of-fold
    error per set; the refit is ForestTrainer().fit(features, target, num_boost_round=best_iteration + 1,
    init_model=init_model, **best_parameters), bit for bit.

    sample_weight: one weight per row (train.validate_sample_weight; DESIGN.md section 9, "Sample weights").  Every fold
    of every set trains with the weights of its training rows, and so does the refit on all rows, which is
    ForestTrainer().fit(..., sample_weight=sample_weight, ...) as above, bit for bit.  `results`, the curves and the
    selection stay on the UNWEIGHTED out-of-fold error and metrics.  A fold whose training rows all weigh 0 is a
    ValueError that names the model.

    monotone_constraints: one sign per feature (train.validate_monotone_constraints; DESIGN.md section 9, "Monotone
    constraints").  Every fold of every set and the refit grow their trees under it; the refit is
    ForestTrainer().fit(..., monotone_constraints=monotone_constraints, ...) as above, bit for bit."""
    started = time.perf_counter()
    sets, per_batch = validate_cross_validation(parameters, n_folds, seed, num_boost_round, early_stopping_rounds,
                                                max_bin, models_per_batch, metrics, select_by)
    metrics, select_by = validate_selection(metrics, select_by)
    in_hbm = isinstance(features, _lib.DeviceArray)
    if in_hbm:
        n_features = _device_columns(features, None)
        n, target = _device_labels(np.asarray(target).reshape(-1).shape[0], target, "training")
        if n > features.shape[0]:
            raise ValueError(f"{n} labels exceed the device matrix's {features.shape[0]} rows")
        device = features.device
    else:
        features, target = _matrix_and_labels(features, target, "training")
        n, n_features = features.shape
    if init_model is not None:
        validate_init_model(init_model, n_features, device)
    if monotone_constraints is not None:
        monotone_constraints = validate_monotone_constraints(monotone_constraints, n_features)
    folds = fold_assignment(groups, n_folds, seed, n)
    if sample_weight is not None:       # every set holds the same folds out: one set's models stand for all
        sample_weight = validate_batch_weight(sample_weight, n, folds, list(range(n_folds)) + [-1], sets)
    if per_batch is None:
        per_batch = _sets_per_batch(n, n_features, in_hbm, sets, n_folds, device, metrics, sample_weight is not None)
    timings = dict.fromkeys(("cuts", "bin", "boost", "refit"), 0.0)
    mark = time.perf_counter()
    cuts = compute_cuts_device(features, n, max_bin, n_features, device) if in_hbm else compute_cuts(features, max_bin)
    timings["cuts"] = (time.perf_counter() - mark) * 1000.0

    def begin(models, metrics=()):
        batch = ForestTrainerBatch(device)
        if in_hbm:
            batch.begin_device(features, n, target, folds, models, n_features, max_bin, cuts, metrics, init_model,
                               sample_weight, monotone_constraints)
        else:
            batch.begin(features, target, folds, models, max_bin, cuts, metrics, init_model, sample_weight,
                        monotone_constraints)
        timings["bin"] += batch.timings["bin"]
        return batch

    fold_history = [None] * len(sets)
    fold_counts = [None] * len(sets)
    initial_errors = [None] * len(sets)
    for first in range(0, len(sets), per_batch):
        chunk = sets[first:first + per_batch]
        batch = begin([dict(one, held_out=k) for one in chunk for k in range(n_folds)], metrics)
        try:
            mark = time.perf_counter()
            summed, rules = [[] for _ in chunk], [FirstMinimum(early_stopping_rounds) for _ in chunk]
            running = np.ones(len(chunk), bool)
            for round_ in range(num_boost_round):
                errors = batch.step(np.repeat(running, n_folds))
                for s in np.nonzero(running)[0]:
                    models = range(s * n_folds, (s + 1) * n_folds)
                    summed[s].append(_selection_score(select_by, errors[s * n_folds:(s + 1) * n_folds],
                                                      [batch.metric_counts[m][-1] for m in models] if metrics else None))
                    if rules[s].see(round_, summed[s][-1]):
                        running[s] = False
                if not running.any():
                    break
            for s in range(len(chunk)):
                fold_history[first + s] = [list(batch.history[s * n_folds + k]) for k in range(n_folds)]
                if init_model is not None:
                    initial_errors[first + s] = sum(batch.initial_errors[s * n_folds:(s + 1) * n_folds])
                if metrics:
                    fold_counts[first + s] = [list(batch.metric_counts[s * n_folds + k]) for k in range(n_folds)]
            timings["boost"] += (time.perf_counter() - mark) * 1000.0
        finally:
            batch.close()
    chosen = select_parameters(fold_history, early_stopping_rounds, select_by, fold_counts if metrics else None)
    import pandas as pd
    results = pd.DataFrame(sets)
    results["best_iteration"], results["error"], results["rounds"] = \
        chosen["best_iteration"], chosen["error"], chosen["rounds"]
    results["fold_errors"] = [[curve[chosen["best_iteration"][p]] for curve in fold_history[p]]
                              for p in range(len(sets))]
    for name in metrics:
        results[name] = [chosen["metrics_history"][p][name][chosen["best_iteration"][p]] for p in range(len(sets))]
    best_set = chosen["chosen"]
    extra = dict(metrics_history=chosen["metrics_history"], fold_metric_counts=fold_counts, select_by=select_by) \
        if metrics else {}
    if init_model is not None:
        results["initial_error"] = initial_errors
        extra["initial_errors"] = initial_errors
    out = CrossValidation(**extra, results=results, history=chosen["history"], fold_history=fold_history, parameters=sets,
                          chosen=best_set, best_parameters=dict(sets[best_set]),
                          best_iteration=chosen["best_iteration"][best_set], folds=folds, timings=timings)
    if refit:
        mark = time.perf_counter()
        batch = begin([dict(sets[best_set], held_out=-1)])
        try:
            for _ in range(out.best_iteration + 1):
                batch.step()
            out.model = batch.model(0)
        finally:
            batch.close()
        timings["refit"] = (time.perf_counter() - mark) * 1000.0
    timings["total"] = (time.perf_counter() - started) * 1000.0
    return out


def row_groups(rows):
    """One group per (kind, query_index) of FeatureEngineering.rows: the candidates sampled for one train title, or
    the generated row of one truth title, never straddle folds."""
    return (rows["kind"].to_numpy().astype(np.int64) << 40) | rows["query_index"].to_numpy().astype(np.int64)


def tune_model_parameters(truth_titles, truth_title_ids, train_titles, train_title_ids, parameters, n_folds=5, top_n=100,
                          sample_n=10, seed=0, device=0, transform=True, cover=False, init_model=None,
                          kind_weights=None, monotone_constraints=None, misspelling_profile=None, **cv_arguments):
    """Parameter search from raw titles in one call: FeatureEngineering(..., no evaluation split).
    generate_device_data_sets() -> cross_validate on the matrix in HBM, folds by row_groups -> the refit model.
    cv_arguments: num_boost_round, early_stopping_rounds, max_bin, models_per_batch, metrics, select_by.  Returns cross_validate's result
    with `rows` (FeatureEngineering.rows), `feature_importance` and the FeatureEngineering stages in `timings`.
    cover: also count the model's cover on the matrix while it is in HBM (ForestModel.fit_cover_device), so that the
    model can explain its predictions; `timings` then has "cover".  init_model: cross_validate's, a ForestModel of
    FEATURES_COUNT features that every fold, set and the refit continue from.  kind_weights: {"generated", "negative",
    "positive"} -> the sample weight of the rows of that kind (training_set.kind_weights; a name left out: 1.0), handed
    to cross_validate as sample_weight.  monotone_constraints: cross_validate's, as FEATURES_COUNT signs or as a dict by
    FEATURE_NAMES (feature_engineering.ratio_constraints()).  misspelling_profile: FeatureEngineering's (None, a
    MisspellingProfile or "fit"); the result's `misspelling_profile` is the profile that was used.  Everything is validated before any device work and everything held in HBM is
    freed on every exit path."""
    from .feature_engineering import FEATURES_COUNT, FEATURE_NAMES
    from .training_set import FeatureEngineering, kind_weights as weights_of_kinds, validate_kind_weights
    started = time.perf_counter()
    unknown = set(cv_arguments) - {"num_boost_round", "early_stopping_rounds", "max_bin", "models_per_batch", "metrics",
                                   "select_by"}
    if unknown:
        raise ValueError(f"unknown cross-validation arguments {sorted(unknown)}")
    validate_cross_validation(parameters, n_folds, seed, **cv_arguments)
    if init_model is not None:
        validate_init_model(init_model, FEATURES_COUNT, device)
    if kind_weights is not None:
        validate_kind_weights(kind_weights)
    if monotone_constraints is not None:
        monotone_constraints = validate_monotone_constraints(monotone_constraints, FEATURES_COUNT, FEATURE_NAMES)
    fe = FeatureEngineering(truth_titles, truth_title_ids, train_titles, train_title_ids, top_n=top_n,
                            sample_n=sample_n, seed=seed, device=device, transform=transform,
                            evaluation_fractions=dict(generated=0.0, negative=0.0, positive=0.0),
                            misspelling_profile=misspelling_profile)
    sets = fe.generate_device_data_sets()
    try:
        matrix = _lib.DeviceArray.view(sets.train.ptr, (sets.n_train, sets.train.shape[1]), np.float32, device)
        out = cross_validate(matrix, sets.train_target, parameters, n_folds=n_folds, groups=row_groups(fe.rows),
                             seed=seed, refit=True, device=device, init_model=init_model,
                             sample_weight=None if kind_weights is None else weights_of_kinds(fe.rows, kind_weights),
                             monotone_constraints=monotone_constraints, **cv_arguments)
        if cover:
            mark = time.perf_counter()
            out.model.fit_cover_device(sets.train, sets.n_train)
            out.timings["cover"] = (time.perf_counter() - mark) * 1000.0
    finally:
        sets.free()
    out.timings = dict(fe.timings, **out.timings)
    out.rows, out.feature_importance = fe.rows, out.model.feature_importance()
    out.misspelling_profile = fe.misspelling_profile
    out.timings["total"] = (time.perf_counter() - started) * 1000.0
    return out
