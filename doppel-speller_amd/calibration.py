"""What the printed probability means: isotonic calibration and the reliability report (DESIGN.md section 9,
"Calibration"; csrc/ds_calibrate.hip).

The model's probability is 1 / (1 + expf(-margin)) of a booster trained with a log loss in which a negative row counts
beta times, on a sampled training set: it ranks, but it is not the share of such pairs that are matches.  A Calibrator
maps the raw score to the match rate observed on labelled rows: the isotonic (non-decreasing) least-squares fit of the
0/1 labels on the score's order, kept as its level sets.  The fit runs on the device on exact integers
(ds_isotonic_fit_device) and is unique, so it repeats bit for bit; the map is a look-up without interpolation, the
same bits on the host (transform) and on the device (transform_device).  raw_threshold(q) turns "accept where the
calibrated value exceeds q" into a probability_threshold for the decision stages, which stay as they are.
reliability() bins a probability against the labels (ds_reliability_device: integer sums per bin) and derives ECE, MCE
and the Brier score on the host.
"""
import numpy as np

from . import _lib

ROWS_MAX = (1 << 31) - 1
BINS_MAX = 256
NAN_KEY = 0xFFFFFFFF
FLT_MAX = np.float32(np.finfo(np.float32).max)
SCALE = float(1 << 30)                             # the quantum of the reliability sums


def cut_key(values):
    """uint32 keys of float32 values (ds_radix.h): ascending keys = ascending values, -0.0 as +0.0, a NaN 0xFFFFFFFF."""
    bits = np.ascontiguousarray(values, dtype=np.float32).view(np.uint32).astype(np.uint64)
    bits = np.where(bits == 0x80000000, 0, bits)
    keys = np.where(bits & 0x80000000, ~bits & 0xFFFFFFFF, bits ^ 0x80000000)
    return np.where((bits & 0x7FFFFFFF) > 0x7F800000, NAN_KEY, keys).astype(np.uint32)


def _vector(name, values, n=None):
    values = np.asarray(values)
    if values.ndim != 1 or (n is not None and values.shape[0] != n):
        expected = "a 1-D array" if n is None else f"{n} values"
        raise ValueError(f"{name} must be {expected}, not shape {values.shape}")
    if values.dtype == object or not (np.issubdtype(values.dtype, np.floating) or
                                      np.issubdtype(values.dtype, np.integer) or values.dtype == bool):
        raise ValueError(f"{name} must be numbers, not {values.dtype}")
    return np.ascontiguousarray(values, dtype=np.float32)


def validate_calibration(scores=None, target=None, n=None, n_bins=10, q=0.5):
    """Every check of this module's entry points, made without the library -> a dict of the cleaned arguments.
    scores: None, or a 1-D array of numbers (float32 after cleaning; NaN and infinite scores are allowed: the rule says
    where they go) of at most 2^31 - 1 values; without scores, n says how many rows lie in HBM.  target: None, or one
    finite number per row (a row is positive iff its target != 0).  n_bins: an integer in [1, 256].  q: a number in
    [0, 1)."""
    if scores is not None:
        scores = _vector("scores", scores)
        if n is not None and n != scores.shape[0]:
            raise ValueError(f"n = {n!r} but scores holds {scores.shape[0]} values")
        n = scores.shape[0]
    if n is not None:
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 0 <= n <= ROWS_MAX:
            raise ValueError(f"n must be an integer in [0, {ROWS_MAX}], not {n!r}")
        n = int(n)
    if target is not None:
        target = _vector("target", target, n)
        if not np.isfinite(target).all():
            raise ValueError(f"target[{int(np.argmin(np.isfinite(target)))}] is not finite")
    if isinstance(n_bins, bool) or not isinstance(n_bins, (int, np.integer)) or not 1 <= n_bins <= BINS_MAX:
        raise ValueError(f"n_bins must be an integer in [1, {BINS_MAX}], not {n_bins!r}")
    try:
        q = float(q)
    except (TypeError, ValueError):
        raise ValueError(f"q must be a number, not {q!r}") from None
    if not 0.0 <= q < 1.0:
        raise ValueError(f"q must be in [0, 1), not {q!r}")
    return dict(scores=scores, target=target, n=n, n_bins=int(n_bins), q=q)


class Calibrator:
    """The level sets of an isotonic fit, in ascending order: lo, hi float32[K] (the smallest and largest score of a
    block), pos, neg int64[K] (its positive and negative rows), values float64[K] = pos / (pos + neg), strictly
    increasing; n_rows, the rows that took part; n_nan, the rows left out for a NaN score; kind, what the score is
    ("probability": the float32 probability of ForestModel.predict)."""

    def __init__(self, lo, hi, pos, neg, n_nan=0, kind="probability"):
        self.lo = np.ascontiguousarray(lo, dtype=np.float32)
        self.hi = np.ascontiguousarray(hi, dtype=np.float32)
        self.pos = np.ascontiguousarray(pos, dtype=np.int64)
        self.neg = np.ascontiguousarray(neg, dtype=np.int64)
        if not (self.lo.ndim == 1 and self.lo.shape == self.hi.shape == self.pos.shape == self.neg.shape):
            raise ValueError("lo, hi, pos and neg must be 1-D arrays of one length")
        if self.lo.shape[0] and ((self.pos < 0).any() or (self.neg < 0).any() or (self.pos + self.neg == 0).any()):
            raise ValueError("every block must hold a row, and no count may be negative")
        self.values = self.pos.astype(np.float64) / np.maximum(self.pos + self.neg, 1).astype(np.float64)
        self.n_rows = int((self.pos + self.neg).sum())
        self.n_nan, self.kind = int(n_nan), str(kind)
        self._device = {}                           # device -> (d_lo, d_value), uploaded on first use

    def __len__(self):
        return self.lo.shape[0]

    def __eq__(self, other):
        if not isinstance(other, Calibrator):
            return NotImplemented
        return (self.kind == other.kind and self.n_nan == other.n_nan and
                self.lo.tobytes() == other.lo.tobytes() and self.hi.tobytes() == other.hi.tobytes() and
                np.array_equal(self.pos, other.pos) and np.array_equal(self.neg, other.neg))

    __hash__ = None

    def values32(self):
        """float32[K]: the values as the map returns them."""
        return self.values.astype(np.float32)

    def transform(self, scores):
        """float32 calibrated values of float32 scores, on the host: the value of the last block whose lo is not above
        the score in key order, 0 below lo[0], NaN for a NaN score (and for every score when there is no block)."""
        scores = np.ascontiguousarray(scores, dtype=np.float32)
        keys = cut_key(scores)
        out = np.full(scores.shape, np.nan, dtype=np.float32)
        if len(self) == 0:
            return out
        at = np.searchsorted(cut_key(self.lo), keys, side="right")
        mapped = np.where(at > 0, self.values32()[np.maximum(at, 1) - 1], np.float32(0))
        return np.where(keys == NAN_KEY, np.float32(np.nan), mapped).astype(np.float32)

    def device_arrays(self, device=0):
        """(d_lo, d_value): the map's two float32[K] arrays in HBM on `device`, uploaded once and kept."""
        if device not in self._device:
            held = max(len(self), 1)                # never a zero-byte allocation
            d_lo, d_value = _lib.DeviceArray((held,), np.float32, device), _lib.DeviceArray((held,), np.float32, device)
            if len(self):
                check = _lib.check
                check(_lib.lib().ds_memcpy_h2d(d_lo.ptr, _lib.pointer(self.lo), self.lo.nbytes, device), "ds_memcpy_h2d")
                value = self.values32()
                check(_lib.lib().ds_memcpy_h2d(d_value.ptr, _lib.pointer(value), value.nbytes, device), "ds_memcpy_h2d")
            self._device[device] = (d_lo, d_value)
        return self._device[device]

    def transform_device(self, d_scores, n, d_out, stream=None, device=0):
        """transform for float32[n] scores in HBM into float32[n] d_out (ds_calibration_apply_device); asynchronous on
        `stream`."""
        n = validate_calibration(n=n)["n"]
        d_lo, d_value = self.device_arrays(device)
        _lib.check(_lib.lib().ds_calibration_apply_device(d_lo.ptr, d_value.ptr, len(self), _lib.pointer(d_scores), n,
                                                          _lib.pointer(d_out), _lib.pointer(stream)),
                   "ds_calibration_apply_device")

    def raw_threshold(self, q):
        """The float32 t for which score > t holds where the calibrated value is > q: nextafter(lo[k], -inf) of the
        first block whose float32 value exceeds q; -FLT_MAX when block 0 does, +FLT_MAX when none does.  Pass it as
        probability_threshold to decide at the calibrated level q."""
        q = validate_calibration(q=q)["q"]
        above = np.nonzero(self.values32().astype(np.float64) > q)[0]
        if above.shape[0] == 0:
            return FLT_MAX
        if above[0] == 0:
            return -FLT_MAX
        return np.nextafter(self.lo[above[0]], np.float32(-np.inf))

    def frame(self):
        """A DataFrame with one row per block: lo, hi, pos, neg, value."""
        import pandas as pd
        return pd.DataFrame({"lo": self.lo, "hi": self.hi, "pos": self.pos, "neg": self.neg, "value": self.values})

    def save(self, path):
        """One .npz with the four arrays, n_nan and kind."""
        with open(path, "wb") as handle:
            np.savez(handle, lo=self.lo, hi=self.hi, pos=self.pos, neg=self.neg, n_nan=np.int64(self.n_nan),
                     kind=np.array(self.kind))

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as data:
            return cls(data["lo"], data["hi"], data["pos"], data["neg"], int(data["n_nan"]), str(data["kind"]))

    def free(self):
        for arrays in self._device.values():
            for array in arrays:
                array.free()
        self._device = {}


class IsotonicFit:
    """fit_isotonic_device's account of one call: the Calibrator and out[4] of ds_isotonic_fit_device (blocks, NaN
    rows, points, the blocks that entered the serial level)."""

    def __init__(self, calibrator, out):
        self.calibrator = calibrator
        self.n_blocks, self.n_nan, self.n_points, self.n_serial = (int(value) for value in out)


def fit_isotonic_device(d_scores, n, d_target, device=0, stream=None, kind="probability", details=False):
    """fit_isotonic for float32[n] scores and float32[n] labels that lie in HBM on `device`: the block arrays are
    allocated next to them and only the K blocks come back.  details: return the IsotonicFit instead."""
    n = validate_calibration(n=n)["n"]
    if n and (d_scores is None or d_target is None):
        raise ValueError("the device scores and their target are missing")
    out = np.zeros(4, np.int64)
    if n == 0:
        fitted = Calibrator(np.zeros(0, np.float32), np.zeros(0, np.float32), np.zeros(0, np.int64),
                            np.zeros(0, np.int64), 0, kind)
        return IsotonicFit(fitted, out) if details else fitted
    held = [_lib.DeviceArray((n,), dtype, device) for dtype in (np.float32, np.float32, np.int64, np.int64)]
    try:
        _lib.check(_lib.lib().ds_isotonic_fit_device(_lib.pointer(d_scores), _lib.pointer(d_target), n, held[0].ptr,
                                                     held[1].ptr, held[2].ptr, held[3].ptr, _lib.pointer(out),
                                                     _lib.pointer(stream)), "ds_isotonic_fit_device")
        blocks = int(out[0])
        fitted = Calibrator(*(array.to_host(blocks) for array in held), int(out[1]), kind)
    finally:
        for array in held:
            array.free()
    return IsotonicFit(fitted, out) if details else fitted


def fit_isotonic(scores, target, device=0, kind="probability"):
    """The isotonic fit of 0/1 labels (target != 0) on float32 scores -> Calibrator.  Rows of equal score are one
    point, a NaN score is counted (n_nan) and left out; everything runs on the device on integers
    (ds_isotonic_fit).  validate_calibration says what is accepted."""
    v = validate_calibration(scores=scores, target=target)
    if v["scores"] is None or v["target"] is None:
        raise ValueError("scores and target are missing")
    n = v["n"]
    lo, hi = np.zeros(n, np.float32), np.zeros(n, np.float32)
    pos, neg, out = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(4, np.int64)
    pointer = _lib.pointer
    _lib.check(_lib.lib().ds_isotonic_fit(pointer(v["scores"] if n else None), pointer(v["target"] if n else None), n,
                                          pointer(lo if n else None), pointer(hi if n else None),
                                          pointer(pos if n else None), pointer(neg if n else None), pointer(out),
                                          device), "ds_isotonic_fit")
    blocks = int(out[0])
    return Calibrator(lo[:blocks], hi[:blocks], pos[:blocks], neg[:blocks], int(out[1]), kind)


class ReliabilityReport:
    """A probability against the labels in n_bins equal-width bins.  counts int64[n_bins + 1, 4]: rows, positives,
    sum rint(p * 2^30) and sum rint((p - y)^2 * 2^30) per bin; the last row holds the rows whose probability is a NaN
    or outside [0, 1] (n_outside), which enter nothing else.  Derived in float64: mean_prediction and observed_rate per
    bin (NaN for an empty bin), ece = sum over bins of rows / n * |observed_rate - mean_prediction|, mce = the largest
    such gap, brier = the mean of (p - y)^2, all over the n rows inside [0, 1] (NaN when there is none)."""

    def __init__(self, counts):
        self.counts = np.asarray(counts, dtype=np.int64)
        if self.counts.ndim != 2 or self.counts.shape[1] != 4 or self.counts.shape[0] < 2:
            raise ValueError(f"counts must be an [n_bins + 1, 4] array, not shape {self.counts.shape}")
        self.n_bins = self.counts.shape[0] - 1
        inside = self.counts[:self.n_bins]
        self.n_outside = int(self.counts[self.n_bins, 0])
        self.n = int(inside[:, 0].sum())
        rows = inside[:, 0].astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            self.mean_prediction = inside[:, 2].astype(np.float64) / SCALE / rows
            self.observed_rate = inside[:, 1].astype(np.float64) / rows
        gaps = np.where(inside[:, 0] > 0, np.abs(self.observed_rate - self.mean_prediction), 0.0)
        if self.n:
            self.ece = float((rows / self.n * gaps).sum())
            self.mce = float(gaps.max())
            self.brier = float(int(inside[:, 3].sum()) / SCALE / self.n)
        else:
            self.ece = self.mce = self.brier = float("nan")

    def frame(self):
        """A DataFrame with one row per bin: low, high, rows, positives, mean_prediction, observed_rate."""
        import pandas as pd
        edges = np.arange(self.n_bins + 1, dtype=np.float64) / self.n_bins
        return pd.DataFrame({"low": edges[:-1], "high": edges[1:], "rows": self.counts[:self.n_bins, 0],
                             "positives": self.counts[:self.n_bins, 1], "mean_prediction": self.mean_prediction,
                             "observed_rate": self.observed_rate})


def reliability_device(d_probabilities, n, d_target, n_bins=10, device=0, stream=None):
    """reliability for float32[n] probabilities and labels in HBM on `device`: only the counters come back."""
    v = validate_calibration(n=n, n_bins=n_bins)
    if v["n"] and (d_probabilities is None or d_target is None):
        raise ValueError("the device probabilities and their target are missing")
    d_out = _lib.DeviceArray((v["n_bins"] + 1, 4), np.int64, device)
    try:
        _lib.check(_lib.lib().ds_reliability_device(_lib.pointer(d_probabilities), _lib.pointer(d_target), v["n"],
                                                    v["n_bins"], d_out.ptr, _lib.pointer(stream)),
                   "ds_reliability_device")
        _lib.check(_lib.lib().ds_stream_sync(_lib.pointer(stream), device), "ds_stream_sync")
        return ReliabilityReport(d_out.to_host())
    finally:
        d_out.free()


def reliability(probabilities, target, n_bins=10, device=0):
    """How far a probability is from the observed rate -> ReliabilityReport.  The bin of p is min(floor(p * n_bins),
    n_bins - 1); the sums are integers computed on the device (ds_reliability_device), the same bits run after run."""
    v = validate_calibration(scores=probabilities, target=target, n_bins=n_bins)
    if v["scores"] is None or v["target"] is None:
        raise ValueError("probabilities and target are missing")
    if v["n"] == 0:
        return reliability_device(None, 0, None, v["n_bins"], device)
    d_probabilities = _lib.DeviceArray.from_host(v["scores"], device)
    d_target = _lib.DeviceArray.from_host(v["target"], device)
    try:
        return reliability_device(d_probabilities, v["n"], d_target, v["n_bins"], device)
    finally:
        d_probabilities.free()
        d_target.free()


def calibrate_option(name, value):
    """ds_calibrate_option, for tests: "max_blocks", "segment_points"."""
    _lib.set_option("ds_calibrate_option", name, value)


def calibrate_rows_device(model, d_rows, n, d_target, n_bins=None, stream=None):
    """ForestModel.calibrate_device and train_model(calibrate=True): the model's probabilities of the first n rows of a
    matrix in HBM, kept in HBM, and their isotonic fit -> (Calibrator, raw ReliabilityReport, calibrated
    ReliabilityReport); the two reports are None without n_bins."""
    n = validate_calibration(n=n)["n"]
    if n_bins is not None:
        n_bins = validate_calibration(n_bins=n_bins)["n_bins"]
    if n == 0:
        fitted = fit_isotonic_device(None, 0, None, model.device)
        empty = None if n_bins is None else reliability_device(None, 0, None, n_bins, model.device)
        return fitted, empty, empty
    d_probabilities = _lib.DeviceArray((n,), np.float32, model.device)
    d_calibrated = None
    try:
        model.predict_device(d_rows, n, None, d_probabilities, stream)
        fitted = fit_isotonic_device(d_probabilities, n, d_target, model.device, stream)
        if n_bins is None:
            return fitted, None, None
        raw = reliability_device(d_probabilities, n, d_target, n_bins, model.device, stream)
        d_calibrated = _lib.DeviceArray((n,), np.float32, model.device)
        fitted.transform_device(d_probabilities, n, d_calibrated, stream, model.device)
        return fitted, raw, reliability_device(d_calibrated, n, d_target, n_bins, model.device, stream)
    finally:
        d_probabilities.free()
        if d_calibrated is not None:
            d_calibrated.free()
