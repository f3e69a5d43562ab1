"""Is a difference real: the paired bootstrap of the evaluation error ("Is a difference real: the
paired bootstrap"; csrc/ds_bootstrap.hip).

Everything the project reports about a model is an integer count over an evaluation set: tp, tn, fp and fn, or the four
outcomes of predictions_accuracy.  Here every row carries an outcome CODE in {0, 1, 2, 3} under each of M prediction
sets (models, thresholds, matchers), the rows are resampled B times with replacement by UNIT (the train title of a row,
a fold group; the row itself without groups), the same draws for every set, and the counts of every replicate come back
as integers.  The error of a replicate is code-2 count + weight * code-1 count (fn + beta * fp, or incorrectly_not_found
+ 5 * incorrectly_matched); an interval is a pair of quantiles of the B errors of a set, and the difference of two sets
is taken replicate by replicate, which is what makes it a paired comparison.  The resampling runs on the device
(ds_bootstrap_counts); the statistics over the B x M numbers are float64 on the host.
"""
import ctypes

import numpy as np

from . import _lib

SETS_MAX = 64
BOOT_MAX = 1 << 16
ROWS_MAX = 1 << 31
PURPOSE_DRAW = 7                                   # DS_BOOTSTRAP_PURPOSE_DRAW
MODEL_CODES = ("tn", "fp", "fn", "tp")             # ds_outcome_codes_device
ACCURACY_CODES = ("correctly_not_found", "incorrectly_matched", "incorrectly_not_found", "correctly_matched")
ACCURACY_WEIGHT = 5.0                              # custom_error = incorrectly_not_found + 5 * incorrectly_matched


def _whole(name, value, low, high):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not low <= value <= high:
        raise ValueError(f"{name} must be an integer in [{low}, {high}], not {value!r}")
    return int(value)


def _real(name, value, low_open, high_open=None):
    try:
        value = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a number, not {value!r}") from None
    if not np.isfinite(value) or value <= low_open or (high_open is not None and value >= high_open):
        bound = f"in ({low_open:g}, {high_open:g})" if high_open is not None else f"finite and above {low_open:g}"
        raise ValueError(f"{name} must be {bound}, not {value!r}")
    return value


def dense_units(groups):
    """groups (any 1-D integer or string array) -> (int32[n] unit numbers, U): the distinct values numbered densely in
    order of first appearance."""
    groups = np.asarray(groups)
    if groups.shape[0] == 0:
        return np.zeros(0, np.int32), 0
    _, first, inverse = np.unique(groups, return_index=True, return_inverse=True)
    rank = np.empty(first.shape[0], np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(first.shape[0])
    return np.ascontiguousarray(rank[inverse.reshape(-1)], dtype=np.int32), int(first.shape[0])


def validate_bootstrap(codes=None, groups=None, n_boot=2000, seed=0, level=0.95, n=None, models=None, n_features=None,
                       threshold=0.9, beta=5.0, names=None):
    """Every check of this module's entry points, made without the library -> a dict of the cleaned arguments.
    codes: None, or an integer [M, n] array (a 1-D array is one set) with 1 <= M <= 64, n <= 2^31 and every code in
    {0, 1, 2, 3}; without codes, n says how many rows there are.  groups: None, or a 1-D integer or string array of n
    values, one per row; an object array passes when every value is a string (`unit`: their dense numbers in order of
    first appearance, `n_units` how many).  n_boot in [1, 65536]; seed in [0, 2^63); level, threshold in (0, 1); beta
    finite and above 0.  models: None, or 1..64 open ForestModels on one device with the same feature count
    (n_features, when given).  names: None, or one distinct string per set."""
    from .forest import ForestModel
    n_sets = None
    if codes is not None:
        codes = np.asarray(codes)
        if codes.ndim == 1:
            codes = codes.reshape(1, -1)
        if codes.ndim != 2:
            raise ValueError(f"codes must be an [M, n] array, not shape {codes.shape}")
        if codes.dtype == bool or not np.issubdtype(codes.dtype, np.integer):
            raise ValueError(f"codes must be integers, not {codes.dtype}")
        n_sets = codes.shape[0]
        if not 1 <= n_sets <= SETS_MAX:
            raise ValueError(f"{n_sets} prediction sets: codes must hold 1 to {SETS_MAX}")
        if n is not None and n != codes.shape[1]:
            raise ValueError(f"n = {n!r} but codes has {codes.shape[1]} rows")
        n = codes.shape[1]
        if codes.size and (codes.min() < 0 or codes.max() > 3):
            at = np.argwhere((codes < 0) | (codes > 3))[0]
            raise ValueError(f"codes[{at[0]}][{at[1]}] = {codes[at[0], at[1]]} is not one of 0, 1, 2, 3")
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
    if models is not None:
        if isinstance(models, ForestModel) or not hasattr(models, "__len__"):
            raise ValueError("models must be a list of ForestModels")
        models = list(models)
        if not 1 <= len(models) <= SETS_MAX:
            raise ValueError(f"{len(models)} models: there must be 1 to {SETS_MAX}")
        for at, model in enumerate(models):
            if not isinstance(model, ForestModel):
                raise ValueError(f"models[{at}] must be a ForestModel, not {type(model).__name__}")
            if not model.handle:
                raise ValueError(f"models[{at}] is closed")
            if n_features is None:
                n_features = model.n_features
            if model.n_features != n_features:
                raise ValueError(f"models[{at}] has {model.n_features} features, not {n_features}")
            if model.device != models[0].device:
                raise ValueError(f"models[{at}] lives on device {model.device}, models[0] on device {models[0].device}")
        n_sets = len(models)
    n = _whole("n", 0 if n is None else n, 0, ROWS_MAX)
    unit, n_units = None, n
    if groups is not None:
        groups = np.asarray(groups)
        if groups.ndim != 1 or groups.shape[0] != n:
            raise ValueError(f"groups must hold {n} values, one per row, not shape {groups.shape}")
        if groups.dtype == object and all(isinstance(value, str) for value in groups):
            groups = groups.astype(str)                # a pandas column of titles (.to_numpy())
        if groups.dtype == bool or not (np.issubdtype(groups.dtype, np.integer) or groups.dtype.kind in "US"):
            raise ValueError(f"groups must be integers or strings (an object array: of strings only), not "
                             f"{groups.dtype}")
        unit, n_units = dense_units(groups)
    n_boot = _whole("n_boot", n_boot, 1, BOOT_MAX)
    seed = _whole("seed", seed, 0, (1 << 63) - 1)
    level = _real("level", level, 0.0, 1.0)
    threshold = _real("threshold", threshold, 0.0, 1.0)
    beta = _real("beta", beta, 0.0)
    if names is not None:
        if isinstance(names, (str, bytes)) or not hasattr(names, "__len__"):
            raise ValueError(f"names must be a sequence of strings, not {names!r}")
        names = tuple(names)
        if not all(isinstance(name, str) for name in names) or len(set(names)) != len(names):
            raise ValueError("names must be distinct strings")
        if n_sets is not None and len(names) != n_sets:
            raise ValueError(f"{len(names)} names for {n_sets} prediction sets")
    return dict(codes=codes, n=n, n_sets=n_sets, unit=unit, n_units=n_units, n_boot=n_boot, seed=seed, level=level,
                models=models, n_features=n_features, threshold=threshold, beta=beta, names=names)


class BootstrapCounts:
    """What bootstrap_counts returns: counts int64[n_boot, M, 4], the outcome counts of every replicate and set;
    baseline int64[M, 4], those of the rows as they are; n_units, the units drawn per replicate; seed."""

    def __init__(self, counts, baseline, n_units, seed=0):
        self.counts = np.asarray(counts, dtype=np.int64)
        self.baseline = np.asarray(baseline, dtype=np.int64)
        self.n_units, self.seed = int(n_units), int(seed)


class ErrorDifference:
    """ErrorBootstrap.difference(a, b): `differences` float64[n_boot] = errors[:, a] - errors[:, b] replicate by
    replicate; `baseline` the difference of the two baseline errors; `mean`; `interval` (low, high) at `level`;
    `standard_error`; share_better = (#{d < 0} + 0.5 * #{d == 0}) / n_boot, the share of replicates in which a has the
    smaller error, ties counted half."""

    def __init__(self, differences, baseline, level):
        d = np.asarray(differences, dtype=np.float64)
        self.differences, self.baseline, self.level = d, float(baseline), float(level)
        self.mean = float(d.mean())
        low, high = np.quantile(d, [(1 - level) / 2, (1 + level) / 2])
        self.interval = (float(low), float(high))
        self.standard_error = float(d.std(ddof=1)) if d.shape[0] > 1 else 0.0
        self.share_better = float((np.count_nonzero(d < 0) + 0.5 * np.count_nonzero(d == 0)) / d.shape[0])


class ErrorBootstrap:
    """The errors of M prediction sets under one paired bootstrap.  counts int64[n_boot, M, 4] and baseline_counts
    int64[M, 4] as BootstrapCounts holds them, with the classes named by `codes` (MODEL_CODES or ACCURACY_CODES);
    errors float64[n_boot, M] = code-2 count + weight * code-1 count per replicate and baseline_errors float64[M]
    likewise (fn + beta * fp; incorrectly_not_found + 5 * incorrectly_matched); standard_error float64[M] =
    errors.std(ddof=1), 0.0 for one replicate; names, n_units, n_boot, seed, weight."""

    def __init__(self, counts, baseline, weight, names=None, n_units=0, seed=0, codes=MODEL_CODES):
        self.counts = np.asarray(counts, dtype=np.int64)
        self.baseline_counts = np.asarray(baseline, dtype=np.int64)
        self.n_boot, self.n_sets = self.counts.shape[0], self.counts.shape[1]
        self.weight, self.n_units, self.seed, self.codes = float(weight), int(n_units), int(seed), tuple(codes)
        self.names = tuple(names) if names is not None else tuple(f"set{m}" for m in range(self.n_sets))
        self.errors = self.counts[:, :, 2].astype(np.float64) + self.weight * self.counts[:, :, 1].astype(np.float64)
        self.baseline_errors = self.baseline_counts[:, 2].astype(np.float64) + \
            self.weight * self.baseline_counts[:, 1].astype(np.float64)
        self.standard_error = self.errors.std(axis=0, ddof=1) if self.n_boot > 1 else np.zeros(self.n_sets)

    def index(self, which):
        """A set given by position or by name -> its position."""
        if isinstance(which, str):
            if which not in self.names:
                raise ValueError(f"{which!r} is not one of the names {self.names}")
            return self.names.index(which)
        return _whole("set", which, 0, self.n_sets - 1)

    def interval(self, level=0.95):
        """float64[M, 2]: np.quantile(errors[:, m], [(1 - level) / 2, (1 + level) / 2]), NumPy's linear method."""
        level = _real("level", level, 0.0, 1.0)
        return np.quantile(self.errors, [(1 - level) / 2, (1 + level) / 2], axis=0).T.copy()

    def difference(self, a, b, level=0.95):
        """Set a against set b (positions or names), replicate by replicate -> ErrorDifference; negative: a is better."""
        a, b, level = self.index(a), self.index(b), _real("level", level, 0.0, 1.0)
        return ErrorDifference(self.errors[:, a] - self.errors[:, b], self.baseline_errors[a] - self.baseline_errors[b],
                               level)

    def frame(self, level=0.95):
        """A DataFrame with one row per set: name, the four baseline counts, baseline_error, mean_error,
        standard_error, low and high of interval(level)."""
        import pandas as pd
        bounds = self.interval(level)
        columns = {"name": list(self.names)}
        for c, code in enumerate(self.codes):
            columns[code] = self.baseline_counts[:, c]
        columns.update(baseline_error=self.baseline_errors, mean_error=self.errors.mean(axis=0),
                       standard_error=self.standard_error, low=bounds[:, 0], high=bounds[:, 1])
        return pd.DataFrame(columns)


SWEEP_CELLS_MAX = 1 << 25                          # n_boot x T x U at most: 32 bytes each, 1 GiB of counts
SWEEP_LEVENSHTEIN_MAX, SWEEP_PROBABILITY_MAX = 101, 256


def validate_sweep_bootstrap(n_boot=0, seed=0, groups=None, n_titles=0, n_levenshtein=1, n_probability=1):
    """The checks of threshold_sweep's bootstrap arguments, made without the library -> dict(n_boot, seed, unit,
    n_units).  n_boot in [0, 65536] (0: no bootstrap); seed in [0, 2^63); groups: None, or a 1-D integer or string
    array with one value per title (`unit`: their dense numbers in order of first appearance; None: every title its own
    unit, n_units = n_titles); n_titles below 2^31; a grid of 1..101 x 1..256 thresholds with n_boot x T x U <= 2^25,
    which keeps the counts (int64[n_boot, T, U, 4], 32 bytes per replicate and cell) at 1 GiB at most."""
    n_boot = _whole("n_boot", n_boot, 0, BOOT_MAX)
    seed = _whole("seed", seed, 0, (1 << 63) - 1)
    n_titles = _whole("n_titles", n_titles, 0, ROWS_MAX - 1)
    T = _whole("n_levenshtein", n_levenshtein, 1, SWEEP_LEVENSHTEIN_MAX)
    U = _whole("n_probability", n_probability, 1, SWEEP_PROBABILITY_MAX)
    if n_boot * T * U > SWEEP_CELLS_MAX:
        raise ValueError(f"n_boot x T x U = {n_boot} x {T} x {U} = {n_boot * T * U} is above 2^25 = {SWEEP_CELLS_MAX}: "
                         f"the counts take 32 bytes per replicate and cell, {32 * n_boot * T * U} bytes here, and 1 GiB "
                         f"(2^25 x 32) is the most")
    try:
        v = validate_bootstrap(groups=groups, n=n_titles)
    except ValueError as error:
        raise ValueError(str(error).replace("per row", "per title")) from None
    return dict(n_boot=n_boot, seed=seed, unit=v["unit"], n_units=v["n_units"])


class SweepBootstrap(ErrorBootstrap):
    """The cells of a threshold sweep under one paired bootstrap of the titles (Prediction.threshold_sweep with
    n_boot > 0; ds_sweep_bootstrap_device): an ErrorBootstrap whose sets are the T x U cells in the frame's order (cell
    = t index x U + u index), with codes = ACCURACY_CODES, weight = 5 and names "t/u".  counts int64[n_boot, T, U, 4]
    and baseline int64[T, U, 4] as the device returns them.  levenshtein_thresholds int64[T] and probability_thresholds
    float64[U] are the shown values; `reference` is the (levenshtein_threshold, probability_threshold) of the
    Prediction that made it, the default cell of `against` when the grid holds it.  share_best float64[C]: the share of
    replicates in which the cell has the smallest error, a replicate's win divided equally among the cells that tie for
    it (sums to 1)."""

    def __init__(self, counts, baseline, levenshtein_thresholds, probability_thresholds, n_units=0, seed=0,
                 reference=None):
        self.levenshtein_thresholds = np.asarray(levenshtein_thresholds, dtype=np.int64).reshape(-1)
        self.probability_thresholds = np.asarray(probability_thresholds, dtype=np.float64).reshape(-1)
        T, U = self.levenshtein_thresholds.shape[0], self.probability_thresholds.shape[0]
        counts = np.asarray(counts, dtype=np.int64)
        names = [f"{int(t)}/{float(u)!r}" for t in self.levenshtein_thresholds for u in self.probability_thresholds]
        super().__init__(counts.reshape(counts.shape[0], T * U, 4), np.asarray(baseline, dtype=np.int64).reshape(T * U, 4),
                         ACCURACY_WEIGHT, names, n_units, seed, ACCURACY_CODES)
        self.reference = None if reference is None else (int(reference[0]), float(reference[1]))
        smallest = self.errors.min(axis=1, keepdims=True)
        ties = self.errors == smallest
        self.share_best = (ties / ties.sum(axis=1, keepdims=True)).sum(axis=0) / self.n_boot

    def cell(self, levenshtein_threshold, probability_threshold):
        """The position of cell (t, u); u is compared as float32, like probability_threshold."""
        t_at = np.flatnonzero(self.levenshtein_thresholds == levenshtein_threshold)
        with np.errstate(over="ignore"):
            u_at = np.flatnonzero(self.probability_thresholds.astype(np.float32) == np.float32(probability_threshold))
        if t_at.shape[0] == 0 or u_at.shape[0] == 0:
            raise ValueError(f"the grid has no cell ({levenshtein_threshold!r}, {probability_threshold!r})")
        return int(t_at[0]) * self.probability_thresholds.shape[0] + int(u_at[0])

    def best(self):
        """The cell with the smallest baseline error; the earlier cell wins a tie."""
        return int(np.argmin(self.baseline_errors))

    def _reference_cell(self, cell):
        if cell is None:
            try:
                return self.best() if self.reference is None else self.cell(*self.reference)
            except ValueError:
                return self.best()
        if isinstance(cell, tuple):
            return self.cell(*cell)
        return self.index(cell)

    def _grid_columns(self):
        U = self.probability_thresholds.shape[0]
        return {"levenshtein_threshold": np.repeat(self.levenshtein_thresholds, U),
                "probability_threshold": np.tile(self.probability_thresholds, self.levenshtein_thresholds.shape[0])}

    def against(self, cell=None, level=0.95):
        """Every cell against one reference cell, replicate by replicate: a DataFrame with one line per cell
        [levenshtein_threshold, probability_threshold, baseline, mean, low, high, share_better], the fields of
        difference(c, cell, level) (negative: the line's cell is better).  cell: a position, a name, a (t, u) pair, or
        None: the instance's own thresholds when the grid holds them, else best()."""
        import pandas as pd
        reference, level = self._reference_cell(cell), _real("level", level, 0.0, 1.0)
        d = self.errors - self.errors[:, reference:reference + 1]
        low, high = np.quantile(d, [(1 - level) / 2, (1 + level) / 2], axis=0)
        columns = self._grid_columns()
        columns.update(baseline=self.baseline_errors - self.baseline_errors[reference], mean=d.mean(axis=0), low=low,
                       high=high, share_better=(np.count_nonzero(d < 0, axis=0) + 0.5 * np.count_nonzero(d == 0, axis=0))
                       / self.n_boot)
        return pd.DataFrame(columns)

    def frame(self, level=0.95):
        """The sweep's frame (prediction.SWEEP_COLUMNS, from the baseline counts) with mean_error, standard_error, low
        and high of interval(level), and share_best."""
        import pandas as pd
        from .prediction import SWEEP_COLUMNS
        bounds = self.interval(level)
        columns = self._grid_columns()
        for name in SWEEP_COLUMNS[2:6]:
            columns[name] = self.baseline_counts[:, ACCURACY_CODES.index(name)]
        columns["custom_error"] = self.baseline_counts[:, 2] + 5 * self.baseline_counts[:, 1]
        columns.update(mean_error=self.errors.mean(axis=0), standard_error=self.standard_error, low=bounds[:, 0],
                       high=bounds[:, 1], share_best=self.share_best)
        return pd.DataFrame(columns)


def sweep_bootstrap_device(d_records, n, levenshtein_thresholds, probability_thresholds, unit, n_units, n_boot, seed,
                           device=0, reference=None):
    """The one call of ds_sweep_bootstrap_device -> SweepBootstrap.  d_records: uint16[n, T] in HBM as
    CandidatePipeline.enqueue_sweep_records fills it; unit: int32[n] on the host or None; the arguments have passed
    validate_sweep_bootstrap with n_boot > 0.  The counts come back once."""
    T, U = len(levenshtein_thresholds), len(probability_thresholds)
    held = [_lib.DeviceArray((n_boot, T, U, 4), np.int64, device), _lib.DeviceArray((T, U, 4), np.int64, device)]
    try:
        if unit is not None and n:
            held.append(_lib.DeviceArray.from_host(unit, device))
        _lib.check(_lib.lib().ds_sweep_bootstrap_device(
            _lib.pointer(d_records if n else None), n, T, U, _lib.pointer(held[2] if len(held) > 2 else None),
            n_units, n_boot, seed, held[0].ptr, held[1].ptr), "ds_sweep_bootstrap_device")
        return SweepBootstrap(held[0].to_host(), held[1].to_host(), levenshtein_thresholds, probability_thresholds,
                              n_units, seed, reference)
    finally:
        for array in held:
            array.free()


def bootstrap_counts(codes, groups=None, n_boot=2000, seed=0):
    """The outcome counts of every bootstrap replicate, resampled on the device (ds_bootstrap_counts) ->
    BootstrapCounts.  codes: integer [M, n], the outcome class 0..3 of row i under prediction set m; groups: the
    resampling unit of every row (None: the row itself).  Replicate b draws n_units units with replacement, a
    closed-form function of (seed, b, position), the same for all sets; the counts are integer sums, the same bits run
    after run.  validate_bootstrap says what is accepted."""
    v = validate_bootstrap(codes=codes, groups=groups, n_boot=n_boot, seed=seed)
    if v["codes"] is None:
        raise ValueError("codes are missing")
    return _counts(v)


def _counts(v):
    """bootstrap_counts after validate_bootstrap: the one call of ds_bootstrap_counts."""
    counts = np.zeros((v["n_boot"], v["n_sets"], 4), np.int64)
    baseline = np.zeros((v["n_sets"], 4), np.int64)
    _lib.check(_lib.lib().ds_bootstrap_counts(_lib.pointer(v["codes"] if v["n"] else None), v["n_sets"], v["n"],
                                              _lib.pointer(v["unit"]), v["n_units"], v["n_boot"], v["seed"],
                                              _lib.pointer(counts), _lib.pointer(baseline)), "ds_bootstrap_counts")
    return BootstrapCounts(counts, baseline, v["n_units"], v["seed"])


def _compare(v, d_rows, d_target, stream):
    """compare_models' device work after validate_bootstrap: every model's margins and codes, then one bootstrap."""
    models, n, n_sets, n_boot = v["models"], v["n"], v["n_sets"], v["n_boot"]
    device = models[0].device
    counts = np.zeros((n_boot, n_sets, 4), np.int64)
    baseline = np.zeros((n_sets, 4), np.int64)
    if n == 0:
        return counts, baseline
    library, pointer, held = _lib.lib(), _lib.pointer, []

    def hold(array):
        held.append(array)
        return array
    try:
        d_margins = hold(_lib.DeviceArray((n,), np.float32, device))
        d_codes = hold(_lib.DeviceArray((n_sets, n), np.uint8, device))
        for m, model in enumerate(models):
            model.predict_device(d_rows, n, d_margins, None, stream)
            _lib.check(library.ds_outcome_codes_device(d_margins.ptr, pointer(d_target), n, v["threshold"],
                                                       ctypes.c_void_p(d_codes.ptr.value + m * n), pointer(stream)),
                       "ds_outcome_codes_device")
        d_unit = hold(_lib.DeviceArray.from_host(v["unit"], device)) if v["unit"] is not None else None
        d_counts = hold(_lib.DeviceArray(counts.shape, np.int64, device))
        d_baseline = hold(_lib.DeviceArray(baseline.shape, np.int64, device))
        _lib.check(library.ds_bootstrap_counts_device(d_codes.ptr, n_sets, n, pointer(d_unit), v["n_units"], n_boot,
                                                      v["seed"], d_counts.ptr, d_baseline.ptr, pointer(stream)),
                   "ds_bootstrap_counts_device")
        return d_counts.to_host(), d_baseline.to_host()
    finally:
        for array in held:
            array.free()


def _target(target, n):
    target = np.asarray(target)
    if target.ndim != 1 or target.shape[0] != n:
        raise ValueError(f"target must hold {n} labels, not shape {target.shape}")
    if target.dtype == object or not np.isin(target, (0, 1)).all():
        raise ValueError("target labels must all be 0 or 1")
    return np.ascontiguousarray(target, dtype=np.float32)


def compare_models_device(models, d_rows, n, d_target, groups=None, n_boot=2000, seed=0, threshold=0.9, beta=5.0,
                          names=None, stream=None):
    """compare_models for the first n rows of a float32 matrix that lies in HBM on the models' device, with its
    float32[n] target in HBM: nothing but the units (4 bytes per row, with groups) goes up and the counts come back."""
    v = validate_bootstrap(groups=groups, n_boot=n_boot, seed=seed, n=n, models=models, threshold=threshold, beta=beta,
                           names=names)
    if v["models"] is None:
        raise ValueError("models are missing")
    if n and (d_rows is None or d_target is None):
        raise ValueError("the device matrix and its target are missing")
    counts, baseline = _compare(v, d_rows, d_target, stream)
    return ErrorBootstrap(counts, baseline, v["beta"], v["names"], v["n_units"], v["seed"], MODEL_CODES)


def compare_models(models, rows, target, groups=None, n_boot=2000, seed=0, threshold=0.9, beta=5.0, names=None):
    """Is model B better?  The evaluation error fn + beta * fp at `threshold` of 1 to 64 ForestModels over the same
    rows under one paired bootstrap -> ErrorBootstrap.  The matrix is uploaded once; every model's predict_device and
    the outcome kernel fill one row of codes in HBM (0 tn, 1 fp, 2 fn, 3 tp, the rule of ds_forest_inspect), then one
    call resamples all of them with the same draws.  groups: the resampling unit of every row, such as the train
    title its candidates were sampled for (tuning.row_groups); None resamples rows.  result.difference(a, b) is the
    replicate-wise difference of two models' errors: its interval and share_better say whether the difference of the
    two baseline errors exceeds what another evaluation sample would give.  validate_bootstrap says what is accepted."""
    rows = np.asarray(rows)
    if rows.ndim != 2:
        raise ValueError(f"rows must be a [n, n_features] matrix, not shape {rows.shape}")
    v = validate_bootstrap(groups=groups, n_boot=n_boot, seed=seed, n=rows.shape[0], models=models,
                           threshold=threshold, beta=beta, names=names)
    if v["models"] is None:
        raise ValueError("models are missing")
    if rows.shape[1] != v["n_features"]:
        raise ValueError(f"rows must be a [n, {v['n_features']}] matrix, not shape {rows.shape}")
    if not (np.issubdtype(rows.dtype, np.floating) or np.issubdtype(rows.dtype, np.integer)):
        raise ValueError(f"rows must be numbers, not {rows.dtype}")
    target = _target(target, v["n"])
    if v["n"] == 0:
        counts, baseline = _compare(v, None, None, None)
    else:
        device = v["models"][0].device
        d_rows = _lib.DeviceArray.from_host(np.ascontiguousarray(rows, dtype=np.float32), device)
        d_target = _lib.DeviceArray.from_host(target, device)
        try:
            counts, baseline = _compare(v, d_rows, d_target, None)
        finally:
            d_rows.free()
            d_target.free()
    return ErrorBootstrap(counts, baseline, v["beta"], v["names"], v["n_units"], v["seed"], MODEL_CODES)


def accuracy_codes(predicted_title_ids, actual_title_ids):
    """uint8[n]: predictions_accuracy's outcome of every title: 0 correctly not found, 1 incorrectly matched,
    2 incorrectly not found, 3 correctly matched."""
    from .prediction import TRAIN_NOT_FOUND_VALUE
    predicted, actual = np.asarray(predicted_title_ids), np.asarray(actual_title_ids)
    if predicted.ndim != 1 or predicted.shape != actual.shape:
        raise ValueError(f"{predicted.reshape(-1).shape[0]} predicted ids but {actual.reshape(-1).shape[0]} actual ids")
    found, same = predicted != TRAIN_NOT_FOUND_VALUE, predicted == actual
    return np.where(found, np.where(same, 3, 1), np.where(same, 0, 2)).astype(np.uint8)


def bootstrap_accuracy(predictions, actual_title_ids, groups=None, n_boot=2000, seed=0):
    """predictions_accuracy under a paired bootstrap -> ErrorBootstrap with ACCURACY_CODES.  predictions: a dict
    (name -> ids) or a list of 1 to 64 arrays of predicted title ids over the same titles, -1 = not found, such as
    generate_test_predictions or one_to_one_matches give under different models or thresholds.  Every title is
    classified on the host by predictions_accuracy's rule; the resampling runs on the device.  baseline_counts and
    baseline_errors are predictions_accuracy of each set; the error is incorrectly_not_found + 5 *
    incorrectly_matched."""
    if isinstance(predictions, dict):
        names, sets = tuple(str(name) for name in predictions), list(predictions.values())
    elif isinstance(predictions, (list, tuple)):
        names, sets = None, list(predictions)
    else:
        raise ValueError("predictions must be a dict or a list of id arrays")
    if not 1 <= len(sets) <= SETS_MAX:
        raise ValueError(f"{len(sets)} prediction sets: there must be 1 to {SETS_MAX}")
    codes = np.stack([accuracy_codes(ids, actual_title_ids) for ids in sets])
    v = validate_bootstrap(codes=codes, groups=groups, n_boot=n_boot, seed=seed, names=names)
    out = _counts(v)
    return ErrorBootstrap(out.counts, out.baseline, ACCURACY_WEIGHT, v["names"], out.n_units, v["seed"], ACCURACY_CODES)
