"""FeatureEngineering.generate_train_and_evaluation_data_sets (doppelspeller/feature_engineering.py:172-378 and
feature_engineering_prepare.py) on the GPU: the training and evaluation sets of the match model from raw titles.

    FeatureEngineering(truth_titles, truth_title_ids, train_titles, train_title_ids)
        .generate_train_and_evaluation_data_sets()   -> (train, train_target, evaluation, evaluation_target)

what ForestTrainer.fit takes.  The rows, in the reference's order (feature_engineering_prepare.py:25-57,
feature_engineering.py:207-274):

    kind 2 (negative)   train rows with id -1, in row order: `sample_n` of their top-n candidates, target 0;
    kind 3 (positive)   per distinct id, in order of first appearance, the LAST train row with that id: `sample_n`
                        candidates, the own truth row in place of the last one when the sample misses it, target 1
                        exactly on the own row;
    kind 1 (generated)  truth rows whose transformed title is longer than 9 characters: the misspelled title against
                        the row itself, target 1.

The device stages: Jaccard top-n of the kind 2 / 3 train rows (TruthIndex), the sample of each (ds_training_pairs_device),
the misspellings (ds_misspell_titles, or ds_misspell_titles_profile with a misspelling_profile), construct_features
of every row into one matrix (two launches).  The split
(_get_evaluation_indexes, feature_engineering.py:277-296) runs on the host with NumPy.  The reference's unseeded
`random` is replaced by per-(seed, purpose, index) streams: the result is a function of the inputs
and `seed`, and does not depend on `chunk_queries`.

Differences from the reference, on purpose: `truth_title_ids` must be unique (as for Prediction); a train id that is
not a truth id is a ValueError (the reference raises KeyError); a kind with fewer rows than its evaluation share is a
ValueError naming the kind (the reference's np.random.choice fails there).
"""
import ctypes
import time

import numpy as np

from . import _lib
from .distributed import slice_queries
from .feature_engineering import (ALLOWED_CHARACTERS, FEATURES_COUNT, MAX_CHARACTERS_ALLOWED_IN_THE_TITLE, SPACE_CODE,
                                  TitleTable, encode_collection)
from .match_maker import validate_index_build
from .forest import ForestModel
from .prediction import (TRAIN_NOT_FOUND_VALUE, StageClock, TruthSide, _CODE_OF, _pack, _validate_chunk, check_characters,
                         default_chunk, transform_or_keep, validate_truth)

KIND_GENERATED, KIND_NEGATIVE, KIND_POSITIVE = 1, 2, 3          # constants.py:46-48
EVALUATION_FRACTIONS = {"generated": 0.05, "negative": 0.10, "positive": 0.05}   # settings.py:47-49
GENERATED_MIN_LENGTH = 9                                          # feature_engineering.py:183-184: longer than 9
MAX_SAMPLE = 16                                                   # the sampler keeps its swap map in registers
MAX_HARD = 16                                                     # mined pairs per title at most (ds_hard_negatives_device)
HARD_COLUMNS = ("query_index", "truth_row", "position", "margin", "probability")
HARD_STAGES = ("top_k", "features", "model", "select", "mined_features", "copy_back")
_TEXT_OF = np.frombuffer(ALLOWED_CHARACTERS.encode("ascii"), dtype=np.uint8)


def _integer(name, value, low, high=None):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < low or \
            (high is not None and value > high):
        bound = f" and at most {high}" if high is not None else ""
        raise ValueError(f"{name} must be an integer of at least {low}{bound}, not {value!r}")
    return int(value)


def validate_training(truth_titles, truth_title_ids, train_titles, train_title_ids, top_n, sample_n, seed,
                      fractions):
    """The constructor's checks (no library needed).  Returns (truth ids, train ids, truth row of every train row
    (-1: not found))."""
    truth_ids = validate_truth(truth_titles, truth_title_ids, top_n)
    ids = np.asarray(train_title_ids)
    if ids.ndim != 1 or len(train_titles) != ids.shape[0]:
        raise ValueError(f"{len(train_titles)} train titles but {ids.reshape(-1).shape[0]} train title ids")
    if ids.shape[0] and not np.issubdtype(ids.dtype, np.integer):
        raise ValueError(f"train title ids must be integers, not {ids.dtype}")
    ids = ids.astype(np.int64)
    if ids.shape[0] and ids.min() < TRAIN_NOT_FOUND_VALUE:
        raise ValueError("train title ids must be truth title ids or -1 (not found)")
    _integer("sample_n", sample_n, 1, MAX_SAMPLE)
    if sample_n > top_n:
        raise ValueError(f"sample_n = {sample_n} exceeds top_n = {top_n}")
    _integer("seed", seed, 0, (1 << 64) - 1)
    for name, fraction in fractions.items():
        if isinstance(fraction, bool) or not isinstance(fraction, (int, float, np.floating, np.integer)) or \
                not 0.0 <= float(fraction) < 1.0:
            raise ValueError(f"the evaluation fraction of {name} rows must lie in [0, 1), not {fraction!r}")
    order = np.argsort(truth_ids, kind="stable")
    found = ids >= 0
    ordered = truth_ids[order]                                # validate_truth: at least top_n >= 1 truth ids
    at = np.minimum(np.searchsorted(ordered, ids[found]), ordered.shape[0] - 1)
    unknown = ordered[at] != ids[found]
    if unknown.any():
        raise ValueError(f"{int(unknown.sum())} train title ids are not truth title ids "
                         f"(first: {int(ids[found][unknown][0])})")
    truth_rows = np.full(ids.shape[0], -1, dtype=np.int64)
    truth_rows[found] = order[at]
    return truth_ids, ids, truth_rows


def validate_hard(model, hard_n, min_margin, exclude_sampled, top_n, sample_n, device=None):
    """The checks of generate_hard_negatives (no library needed) -> (hard_n, min_margin as a float, -inf for None):
    `model` an open ForestModel of 66 features (on `device`, when given), hard_n an integer in 1 .. 16 and at most
    top_n, min_margin None or a finite real, exclude_sampled a bool."""
    if not isinstance(model, ForestModel):
        raise ValueError(f"model must be a ForestModel, not {type(model).__name__}")
    if not model.handle:
        raise ValueError("model is closed")
    if model.n_features != FEATURES_COUNT:
        raise ValueError(f"model has {model.n_features} features, construct_features makes {FEATURES_COUNT}")
    if device is not None and model.device != device:
        raise ValueError(f"model lives on device {model.device}, the training set on device {device}")
    hard_n = _integer("hard_n", hard_n, 1, MAX_HARD)
    if hard_n > top_n:
        raise ValueError(f"hard_n = {hard_n} exceeds top_n = {top_n}")
    if min_margin is not None:
        if isinstance(min_margin, bool) or not isinstance(min_margin, (int, float, np.integer, np.floating)) or \
                not np.isfinite(min_margin):
            raise ValueError(f"min_margin must be None or a finite number, not {min_margin!r}")
    if not isinstance(exclude_sampled, (bool, np.bool_)):
        raise ValueError(f"exclude_sampled must be a bool, not {exclude_sampled!r}")
    if exclude_sampled and sample_n > MAX_SAMPLE:
        raise ValueError(f"exclude_sampled holds sample_n = {sample_n} rows per title, at most {MAX_SAMPLE}")
    return hard_n, float("-inf") if min_margin is None else float(min_margin)


def row_plan(truth_rows):
    """The train rows that produce training rows (feature_engineering_prepare.py:33-55 read through the dicts of
    feature_engineering.py:207-274): (negative rows in row order, per distinct truth row in order of first appearance
    the last train row holding it)."""
    truth_rows = np.asarray(truth_rows, dtype=np.int64)
    negative = np.nonzero(truth_rows < 0)[0]
    rows = np.nonzero(truth_rows >= 0)[0]
    values = truth_rows[rows]
    _, first = np.unique(values, return_index=True)
    _, last_reversed = np.unique(values[::-1], return_index=True)
    last = rows[values.shape[0] - 1 - last_reversed]          # same (sorted) value order as `first`
    positive = last[np.argsort(first, kind="stable")]
    return negative.astype(np.int64), positive.astype(np.int64)


def evaluation_split(kind, seed, fractions=None):
    """_get_evaluation_indexes (feature_engineering.py:277-296) with np.random.default_rng(seed): int(N * fraction)
    rows of each kind drawn without replacement (generated, negative, positive, in that order).  Returns (train rows,
    evaluation rows), both ascending."""
    fractions = dict(EVALUATION_FRACTIONS, **(fractions or {}))
    kind = np.asarray(kind)
    n = kind.shape[0]
    rng = np.random.default_rng(seed)
    chosen = []
    for name, code in (("generated", KIND_GENERATED), ("negative", KIND_NEGATIVE), ("positive", KIND_POSITIVE)):
        candidates = np.nonzero(kind == code)[0]
        size = int(n * fractions[name])
        if size > candidates.shape[0]:
            raise ValueError(f"the evaluation set needs {size} {name} rows, there are {candidates.shape[0]}")
        chosen.append(rng.choice(candidates, size, replace=False))
    evaluation = np.unique(np.concatenate(chosen)).astype(np.int64)
    train = np.setdiff1d(np.arange(n, dtype=np.int64), evaluation)
    return train, evaluation


KIND_CODES = {"generated": KIND_GENERATED, "negative": KIND_NEGATIVE, "positive": KIND_POSITIVE}


def validate_kind_weights(weights):
    """A dict over the names "generated", "negative", "positive" -> {name: float}, 1.0 for a name left out.  Every
    weight is a finite number >= 0; an unknown name is a ValueError."""
    if not isinstance(weights, dict):
        raise ValueError(f"kind weights must be a dict over {sorted(KIND_CODES)}, not {weights!r}")
    unknown = set(weights) - set(KIND_CODES)
    if unknown:
        raise ValueError(f"unknown kind weights {sorted(unknown, key=str)}; known: {sorted(KIND_CODES)}")
    out = {}
    for name in KIND_CODES:
        value = weights.get(name, 1.0)
        if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)) or \
                not np.isfinite(value) or value < 0:
            raise ValueError(f"the weight of {name} rows must be a finite number >= 0, not {value!r}")
        out[name] = float(value)
    return out


def kind_weights(rows, weights):
    """The float32 sample weights of the TRAINING rows of a FeatureEngineering.rows frame, in the order of the
    training matrix (the frame's rows outside the evaluation set, in frame order): weights[name] for a row of that kind
    (validate_kind_weights: "generated", "negative", "positive"; a name left out weighs 1.0).  What
    ForestTrainer.fit_device(..., sample_weight=...) takes for the matrix of generate_device_data_sets."""
    weights = validate_kind_weights(weights)
    kind = np.asarray(rows["kind"])
    training = ~np.asarray(rows["evaluation"]).astype(bool)
    table = np.ones(int(max(KIND_CODES.values())) + 1, np.float32)
    for name, code in KIND_CODES.items():
        table[code] = weights[name]
    if kind.shape[0] and (kind.min() < 1 or kind.max() >= table.shape[0]):
        raise ValueError("rows holds a kind that is not generated (1), negative (2) or positive (3)")
    return np.ascontiguousarray(table[kind.astype(np.int64)][training])


class _DeviceTitles:
    """A ds_titles table made on the device (ds_misspell_titles)."""

    def __init__(self, handle, n):
        self.handle, self.n = handle, n

    def read(self):
        """The rows as (uint8[n, 255] codes, uint8[n] lengths)."""
        enc = np.empty((self.n, MAX_CHARACTERS_ALLOWED_IN_THE_TITLE), dtype=np.uint8)
        lengths = np.empty(self.n, dtype=np.uint8)
        _lib.check(_lib.lib().ds_titles_read(self.handle, _lib.pointer(enc), _lib.pointer(lengths)), "ds_titles_read")
        return enc, lengths

    def strings(self):
        enc, lengths = self.read()
        return [_TEXT_OF[enc[i, :lengths[i]]].tobytes().decode("ascii") for i in range(self.n)]

    def close(self):
        if self.handle:
            _lib.lib().ds_titles_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def validate_profile_argument(misspelling_profile):
    """The misspelling_profile argument of FeatureEngineering, train_model, tune_model_parameters and refresh_model (no
    library needed): None (the reference's generator), a MisspellingProfile that validate_misspelling_profile accepts, or
    "fit": learn it from the call's own labelled train pairs first."""
    from .edits import MisspellingProfile, validate_misspelling_profile
    if misspelling_profile is None or (isinstance(misspelling_profile, str) and misspelling_profile == "fit"):
        return misspelling_profile
    if not isinstance(misspelling_profile, MisspellingProfile):
        raise ValueError(f'misspelling_profile must be None, "fit" or a MisspellingProfile, not {misspelling_profile!r}')
    validate_misspelling_profile(misspelling_profile)
    return misspelling_profile


def misspell_table(source, rows, seed, device=0, stream=None, profile=None):
    """ds_misspell_titles: a device table whose row i misspells row rows[i] of the TitleTable `source` (rows None:
    every row, in order).  With a MisspellingProfile: ds_misspell_titles_profile (the null stream)."""
    if profile is not None:
        from .edits import misspell_profile_table
        return _DeviceTitles(*misspell_profile_table(source, rows, seed, profile, device))
    n = source.n if rows is None else int(np.asarray(rows).shape[0])
    d_rows = None if rows is None else _lib.DeviceArray.from_host(np.ascontiguousarray(rows, dtype=np.int32), device)
    handle = ctypes.c_void_p()
    _lib.check(_lib.lib().ds_misspell_titles(source.handle, _lib.pointer(d_rows), n, ctypes.c_uint64(seed),
                                             _lib.pointer(stream), ctypes.byref(handle)), "ds_misspell_titles")
    return _DeviceTitles(handle, n)


def generate_misspelled_names(titles, seed=0, device=0, profile=None):
    """generate_misspelled_name (feature_engineering_prepare.py:165-173) of every transformed title, title i drawn from
    the purpose-1 stream of index i: a list of str.  profile: a MisspellingProfile (edits.fit_misspelling_profile): the
    titles are misspelled after it instead (ds_misspell_titles_profile, the purpose-8 stream of index i); None makes
    exactly the call made without it."""
    titles = [str(t) for t in titles]
    _integer("seed", seed, 0, (1 << 64) - 1)
    if profile is not None:
        from .edits import validate_misspelling_profile
        validate_misspelling_profile(profile)
    for title in titles:
        if not 3 <= len(title) <= MAX_CHARACTERS_ALLOWED_IN_THE_TITLE or not title.strip():
            raise ValueError(f"not a transformed title (3..255 characters, not all spaces): {title!r}")
    if not titles:
        return []
    chars, offsets = _pack(titles)
    check_characters(chars, offsets, "the")
    enc, lengths = encode_collection(chars, offsets, _CODE_OF)
    return misspell_table(TitleTable(enc, lengths, None, device), None, seed, device, profile=profile).strings()


class DeviceDataSets:
    """The training and evaluation sets with their feature matrices in HBM (FeatureEngineering.
    generate_device_data_sets): `train` / `evaluation` are DeviceArrays float32[max(rows, 1), 66] of which the first
    n_train / n_evaluation rows count, `train_target` / `evaluation_target` host float32 labels.  `features` is the
    full matrix (n_rows rows) when it was kept, else None."""

    def __init__(self, train, n_train, train_target, evaluation, n_evaluation, evaluation_target, misspelled, features,
                 n_rows):
        self.train, self.n_train, self.train_target = train, int(n_train), train_target
        self.evaluation, self.n_evaluation, self.evaluation_target = evaluation, int(n_evaluation), evaluation_target
        self.features, self.n_rows = features, int(n_rows)
        self._misspelled = misspelled

    def to_host(self):
        """(train, train_target, evaluation, evaluation_target) as generate_train_and_evaluation_data_sets returns
        them."""
        return (self.train.to_host(self.n_train), self.train_target, self.evaluation.to_host(self.n_evaluation),
                self.evaluation_target)

    def misspelled_titles(self):
        """The queries of the kind 1 rows, in order, decoded from the device table."""
        return self._misspelled.strings() if self._misspelled is not None else []

    def with_hard_negatives(self, hard):
        """A new DeviceDataSets whose training matrix in HBM is this one's rows followed by the mined rows of `hard`
        (a DeviceHardNegatives), its train_target extended by their zeros; the evaluation part is a copy of this one's.
        Device copies only: ForestTrainer.fit_device(..., init_model=model) takes the result without the matrix leaving
        HBM.  The new object owns its matrices (free() of either leaves the other whole); the misspelled titles and a
        kept `features` stay with this one."""
        if not isinstance(hard, DeviceHardNegatives):
            raise ValueError(f"hard must be a DeviceHardNegatives, not {type(hard).__name__}")
        device, row_bytes = self.train.device, FEATURES_COUNT * 4
        if hard.features.device != device:
            raise ValueError(f"the mined rows live on device {hard.features.device}, the training set on device {device}")
        library, n = _lib.lib(), self.n_train + hard.n
        train = _lib.DeviceArray((max(n, 1), FEATURES_COUNT), np.float32, device)
        evaluation = _lib.DeviceArray((max(self.n_evaluation, 1), FEATURES_COUNT), np.float32, device)
        for target, offset, source, rows in ((train, 0, self.train, self.n_train), (train, self.n_train, hard.features, hard.n),
                                             (evaluation, 0, self.evaluation, self.n_evaluation)):
            if rows:
                _lib.check(library.ds_memcpy_d2d_async(ctypes.c_void_p(target.ptr.value + offset * row_bytes), source.ptr,
                                                       rows * row_bytes, device, None), "ds_memcpy_d2d_async")
        _lib.check(library.ds_stream_sync(None, device), "ds_stream_sync")
        return DeviceDataSets(train, n, np.concatenate((self.train_target, hard.target)).astype(np.float32), evaluation,
                              self.n_evaluation, self.evaluation_target, None, None, self.n_rows + hard.n)

    def free(self):
        """Frees the matrices in HBM (the labels stay)."""
        for array in (self.train, self.evaluation, self.features):
            if array is not None:
                array.free()
        if self._misspelled is not None:
            self._misspelled.close()


class DeviceHardNegatives:
    """The mined rows with their feature matrix in HBM (FeatureEngineering.generate_device_hard_negatives): `features`
    is a DeviceArray float32[max(n, 1), 66] of which the first n rows count, `target` the host float32[n] labels, all
    zeros: every mined row is a negative."""

    def __init__(self, features, n):
        self.features, self.n = features, int(n)
        self.target = np.zeros(self.n, dtype=np.float32)

    def to_host(self):
        """(features float32[n, 66], target float32[n]) as generate_hard_negatives returns them."""
        return self.features.to_host(self.n), self.target

    def free(self):
        self.features.free()


class FeatureEngineering:
    """FeatureEngineering(truth_titles, truth_title_ids, train_titles, train_title_ids).
    generate_train_and_evaluation_data_sets() -> (train, train_target, evaluation, evaluation_target), float32.

    Titles are raw strings put through transform_titles unless transform=False.  train_title_ids: the truth id of
    every train title, -1 where it has none.  top_n: candidates per train title (settings.py:59, 100), sample_n: of
    which sampled (settings.py:58, 10; at most 16).  seed: the streams of the misspellings and the samples, and the
    NumPy generator of the split.  chunk_queries: train titles per top-n pass (default: what a quarter of the free HBM
    holds); the result does not depend on it.  evaluation_fractions: {"generated", "negative", "positive"} -> share
    of ALL rows drawn into the evaluation set (settings.py:47-49).  build_index: "host" or "device", passed to TruthSide.
    misspelling_profile: None, or a MisspellingProfile after which the kind 1 rows are misspelled
    (ds_misspell_titles_profile) instead of after the reference's rule, or "fit": fit_misspelling_profile() of this
    object's own labelled train rows, made by the first call that generates rows and kept as `misspelling_profile`.
    `timings` then has "misspell_profile" (and "misspell_profile_fit"); the kind 2 / 3 rows do not depend on it.

    After a call: `rows` (DataFrame: kind, query_index = train row for kinds 2 / 3 and truth row for kind 1,
    truth_row, target, evaluation), `misspelled_titles` (the queries of the kind 1 rows, in order), `features` (every
    row's construct_features) and `timings` (milliseconds per stage).  generate_device_data_sets() is the form that
    leaves the matrices in HBM (DeviceDataSets).

    generate_hard_negatives(model) / generate_device_hard_negatives(model) mine, for the same train titles, the wrong
    candidates `model` likes best (this project's own, DESIGN.md section 8 "Hard negatives"); they fill `hard_rows` and
    `hard_timings` and leave `rows`, `features` and `timings` alone."""

    def __init__(self, truth_titles, truth_title_ids, train_titles, train_title_ids, top_n=100, sample_n=10, seed=0,
                 device=0, transform=True, chunk_queries=None, evaluation_fractions=None, build_index="host",
                 misspelling_profile=None):
        validate_index_build(build_index, "build_index")
        self.misspelling_profile = validate_profile_argument(misspelling_profile)
        truth_titles, train_titles = list(truth_titles), list(train_titles)
        unknown = set(evaluation_fractions or {}) - set(EVALUATION_FRACTIONS)
        if unknown:
            raise ValueError(f"unknown evaluation fractions {sorted(unknown)}; known: {sorted(EVALUATION_FRACTIONS)}")
        self.evaluation_fractions = dict(EVALUATION_FRACTIONS, **(evaluation_fractions or {}))
        self.truth_title_ids, self.train_title_ids, self.train_truth_rows = validate_training(
            truth_titles, truth_title_ids, train_titles, train_title_ids, top_n, sample_n, seed,
            self.evaluation_fractions)
        _validate_chunk(chunk_queries)
        self.top_n, self.sample_n, self.seed = int(top_n), int(sample_n), int(seed)
        self.device, self.transform, self.chunk_queries = device, transform, chunk_queries
        self._raw_truth, self._raw_train = truth_titles, train_titles
        self.build_index = build_index
        self._truth = self._queries = None
        self.rows = self.misspelled_titles = self.features = None
        self.timings = {}
        self.hard_rows, self.hard_timings = None, {}

    def generate_train_and_evaluation_data_sets(self):
        """feature_engineering.py:321-378: (train, train_target, evaluation, evaluation_target)."""
        timings = dict.fromkeys(("host_prepare", "truth_side", "top_k", "sample_pairs", "misspell", "features",
                                 "copy_back", "split"), 0.0)
        stage = self._device_stages(timings)
        d_features, n_rows, misspelled = stage["d_features"], stage["n_rows"], stage["misspelled"]

        mark = time.perf_counter()
        features = d_features.to_host(n_rows)
        pair_t, target = self._pairs_to_host(stage)
        self.misspelled_titles = misspelled.strings() if misspelled is not None else []
        timings["copy_back"] = (time.perf_counter() - mark) * 1000.0

        # ---- rows and the split
        mark = time.perf_counter()
        target, train_rows, evaluation_rows = self._rows_and_split(stage, pair_t, target)
        self.features = features
        out = (features[train_rows], target[train_rows], features[evaluation_rows], target[evaluation_rows])
        timings["split"] = (time.perf_counter() - mark) * 1000.0
        self.timings = timings
        return out

    def generate_device_data_sets(self, keep_features=False):
        """generate_train_and_evaluation_data_sets with the feature matrix left in HBM -> DeviceDataSets: the same
        stages up to and including the features launches; the pairs' truth rows and targets come back (8 B per row)
        and fill `rows` exactly as on the host path; evaluation_split needs only the kinds; its two index arrays are
        uploaded and two ds_gather_rows_device calls make the contiguous training and evaluation matrices.  The full
        matrix is freed unless keep_features (then DeviceDataSets.features holds it).  The misspelled titles stay
        encoded on the device (DeviceDataSets.misspelled_titles() decodes them on demand); `features` and
        `misspelled_titles` of this object stay None on this path.  `timings` has no copy_back of the features; it
        gains `gather`."""
        timings = dict.fromkeys(("host_prepare", "truth_side", "top_k", "sample_pairs", "misspell", "features",
                                 "copy_back", "split", "gather"), 0.0)
        stage = self._device_stages(timings)
        d_features, n_rows, device = stage["d_features"], stage["n_rows"], self.device

        mark = time.perf_counter()
        pair_t, target = self._pairs_to_host(stage)
        timings["copy_back"] = (time.perf_counter() - mark) * 1000.0
        mark = time.perf_counter()
        target, train_rows, evaluation_rows = self._rows_and_split(stage, pair_t, target)
        self.features = self.misspelled_titles = None
        timings["split"] = (time.perf_counter() - mark) * 1000.0

        mark = time.perf_counter()
        parts = []
        for rows in (train_rows, evaluation_rows):
            d_part = _lib.DeviceArray((max(rows.shape[0], 1), FEATURES_COUNT), np.float32, device)
            if rows.shape[0]:
                d_index = _lib.DeviceArray.from_host(rows.astype(np.int64), device)
                _lib.check(_lib.lib().ds_gather_rows_device(d_features.ptr, FEATURES_COUNT, d_index.ptr, rows.shape[0],
                                                            n_rows, d_part.ptr, None), "ds_gather_rows_device")
                d_index.free()
            parts.append(d_part)
        if not keep_features:
            d_features.free()
        timings["gather"] = (time.perf_counter() - mark) * 1000.0
        self.timings = timings
        return DeviceDataSets(parts[0], train_rows.shape[0], target[train_rows], parts[1], evaluation_rows.shape[0],
                              target[evaluation_rows], stage["misspelled"], d_features if keep_features else None, n_rows)

    def _truth_side(self, timings, started):
        """The TruthSide of this object, made by the first call that needs it (its times go to `timings`)."""
        if self._truth is None:
            self.truth_titles = transform_or_keep(self._raw_truth, self.transform)
            self.train_titles = transform_or_keep(self._raw_train, self.transform)
            timings["host_prepare"] += (time.perf_counter() - started) * 1000.0
            mark = time.perf_counter()
            self._truth = TruthSide(self.truth_titles, self.device, build_index=self.build_index)
            timings["truth_side"] = (time.perf_counter() - mark) * 1000.0
        return self._truth

    def fit_misspelling_profile(self, max_edits=4):
        """The MisspellingProfile of this object's labelled pairs: every train row with a truth id against its truth
        row (edits.fit_misspelling_profile of those pairs), aligned on the device against the truth table that is
        already in HBM; the labelled train titles are uploaded for it once (the query table holds only the rows that
        produce training rows)."""
        from .edits import COUNTS, MisspellingProfile, _max_edits, fit_tables
        max_edits = _max_edits(max_edits)
        truth = self._truth_side(dict(host_prepare=0.0), time.perf_counter())
        labelled = np.nonzero(self.train_truth_rows >= 0)[0]
        if not labelled.shape[0]:
            return MisspellingProfile(np.zeros(COUNTS, np.int64), max_edits)
        chars, offsets = _pack([self.train_titles[i] for i in labelled])
        check_characters(chars, offsets, "train")
        enc, lengths = encode_collection(chars, offsets, _CODE_OF)
        table = TitleTable(enc, lengths, None, self.device)
        d_rows = _lib.DeviceArray.from_host(self.train_truth_rows[labelled].astype(np.int32), self.device)
        try:
            return fit_tables(truth.table, d_rows, table, None, labelled.shape[0], max_edits, self.device)
        finally:
            d_rows.free()
            table.close()

    def _selected_queries(self):
        """The train rows that produce rows (kinds 2 and 3, in that order) as queries of the truth side, made once:
        (negative, positive, selected, own truth rows int32, q_rowptr, q_cols, q_maxint, their TitleTable); the last
        four are None when no train row is selected."""
        if self._queries is None:
            negative, positive = row_plan(self.train_truth_rows)
            selected = np.concatenate((negative, positive))
            own = self.train_truth_rows[selected].astype(np.int32)
            rows = (None, None, None, None)
            if selected.shape[0]:
                chars, offsets = _pack([self.train_titles[i] for i in selected])
                check_characters(chars, offsets, "train")
                enc, lengths = encode_collection(chars, offsets, _CODE_OF)
                rows = self._truth.query_rows(chars, offsets) + (TitleTable(enc, lengths, None, self.device),)
            self._queries = (negative, positive, selected, own) + rows
        return self._queries

    def generate_hard_negatives(self, model, hard_n=5, min_margin=None, exclude_sampled=True):
        """The hard negatives of `model` -> (features float32[m, 66], target float32[m], all zeros).  For every train
        title of the base set (the kind 2 and kind 3 rows, in that order) all top_n candidates are scored by the model
        on the device, and the hard_n (1 .. 16) with the highest margins are kept that are not the title's own truth
        row, whose margin is above min_margin (None: no threshold; log(9) is the margin of probability 0.9: then only
        the false positives of the decision rule are mined) and, with exclude_sampled, that the base set did not draw
        for the title (so base set plus mined rows hold no (title, truth row) pair twice; this needs the base set
        generated by this object first).  Equal margins go to the candidate that is earlier in the Jaccard order.  The
        result does not depend on chunk_queries.  Only the mined pairs and their features travel back.

        After a call: `hard_rows` (DataFrame: query_index = train row, truth_row, position in the Jaccard list, margin,
        probability = the float32 sigmoid of the margin) and `hard_timings` (milliseconds per stage); `rows`,
        `features` and `timings` of the base set are left alone."""
        hard = self.generate_device_hard_negatives(model, hard_n, min_margin, exclude_sampled)
        mark = time.perf_counter()
        out = hard.to_host()
        hard.free()
        self.hard_timings["copy_back"] += (time.perf_counter() - mark) * 1000.0
        return out

    def generate_device_hard_negatives(self, model, hard_n=5, min_margin=None, exclude_sampled=True):
        """generate_hard_negatives with the mined feature matrix left in HBM -> DeviceHardNegatives, for
        DeviceDataSets.with_hard_negatives.  Per chunk of titles every stage is enqueued on the device: the top_n rows,
        construct_features of every (title, candidate), the model's margins, the selection
        (ds_hard_negatives_device), which appends to four dense arrays in HBM behind a running total.  After the last
        chunk the total is read, one construct_features call over the mined pairs makes their matrix (at most hard_n /
        top_n of the work of the first), and the four mined arrays come back for `hard_rows`."""
        hard_n, threshold = validate_hard(model, hard_n, min_margin, exclude_sampled, self.top_n, self.sample_n,
                                          self.device)
        if exclude_sampled and self.rows is None:
            raise ValueError("exclude_sampled=True leaves out the pairs the base set drew: generate the base set with "
                             "this object first, or pass exclude_sampled=False")
        import pandas as pd
        device, k = self.device, self.top_n
        timings = dict.fromkeys(HARD_STAGES, 0.0)
        truth = self._truth_side(dict(host_prepare=0.0), time.perf_counter())
        n_truth = truth.table.n
        _, _, selected, own, q_rowptr, q_cols, q_maxint, query_table = self._selected_queries()
        n_selected = selected.shape[0]
        n_exclude = self.sample_n if exclude_sampled else 0
        if exclude_sampled:
            sampled = self.rows["truth_row"].to_numpy()[:n_selected * n_exclude]
            if self.rows.shape[0] < n_selected * n_exclude or \
                    not np.array_equal(self.rows["query_index"].to_numpy()[:n_selected * n_exclude],
                                       np.repeat(selected, n_exclude)):
                raise ValueError("`rows` is not the base set of this object: generate the base set first, or pass "
                                 "exclude_sampled=False")
            sampled = np.ascontiguousarray(sampled.reshape(n_selected, n_exclude), dtype=np.int32)

        library, clock = _lib.lib(), StageClock(timings, device)
        capacity = n_selected * hard_n
        d_total = _lib.DeviceArray.from_host(np.zeros(1, np.int64), device)
        mined = [_lib.DeviceArray((max(capacity, 1),), dtype, device) for dtype in (np.int32, np.int32, np.int32, np.float32)]
        if n_selected:
            chunk = min(n_selected, self.chunk_queries or default_chunk(device, k * (FEATURES_COUNT * 4 + 8) + 80))
            d_rows = _lib.DeviceArray((chunk, k), np.int32, device)
            d_features = _lib.DeviceArray((chunk * k, FEATURES_COUNT), np.float32, device)
            d_margins = _lib.DeviceArray((chunk * k,), np.float32, device)
            d_offsets = _lib.DeviceArray((chunk,), np.int64, device)
            d_own = _lib.DeviceArray.from_host(own, device)
            for first in range(0, n_selected, chunk):
                last = min(n_selected, first + chunk)
                n = last - first
                rowptr, cols, maxint = slice_queries(q_rowptr, q_cols, q_maxint, first, last)
                d_rowptr = _lib.DeviceArray.from_host(rowptr, device)
                d_cols = _lib.DeviceArray.from_host(cols if cols.shape[0] else np.zeros(1, np.int32), device)
                d_maxint = _lib.DeviceArray.from_host(maxint, device)
                d_exclude = _lib.DeviceArray.from_host(sampled[first:last], device) if n_exclude else None
                clock.device("top_k", lambda: truth.index.top_k_device(d_rowptr, d_cols, d_maxint, n, k, d_rows))
                truth.index.sync()
                clock.device("features", lambda: _lib.check(library.ds_construct_features_indexed_device(
                    query_table.handle, truth.table.handle, None, d_rows.ptr, first, k, SPACE_CODE, n_truth, n * k,
                    d_features.ptr, None), "ds_construct_features_indexed_device"))
                clock.device("model", lambda: model.predict_device(d_features, n * k, d_margins, None))
                clock.device("select", lambda: _lib.check(library.ds_hard_negatives_device(
                    d_rows.ptr, d_margins.ptr, n, k, n_truth, ctypes.c_void_p(d_own.ptr.value + 4 * first),
                    _lib.pointer(d_exclude), n_exclude, hard_n, ctypes.c_float(threshold), first, d_offsets.ptr,
                    d_total.ptr, capacity, *(a.ptr for a in mined), None), "ds_hard_negatives_device"))
                clock.collect()
            for array in (d_rows, d_features, d_margins, d_offsets, d_own):
                array.free()
        total = ctypes.c_int64(0)
        _lib.check(library.ds_hard_total(d_total.ptr, ctypes.byref(total), None), "ds_hard_total")
        m = int(total.value)

        d_mined = _lib.DeviceArray((max(m, 1), FEATURES_COUNT), np.float32, device)
        if m:
            clock.device("mined_features", lambda: _lib.check(library.ds_construct_features_indexed_device(
                query_table.handle, truth.table.handle, mined[0].ptr, mined[1].ptr, 0, 1, SPACE_CODE, n_truth, m,
                d_mined.ptr, None), "ds_construct_features_indexed_device"))
            clock.collect()
        with clock.host("copy_back"):
            pair_q, pair_t, position, margin = (a.to_host(m) for a in mined)
        for array in mined + [d_total]:
            array.free()
        with np.errstate(over="ignore"):
            probability = (np.float32(1.0) / (np.float32(1.0) + np.exp(-margin))).astype(np.float32)
        self.hard_rows = pd.DataFrame(dict(zip(HARD_COLUMNS, (selected[pair_q].astype(np.int64), pair_t.astype(np.int64),
                                                              position, margin, probability))))
        self.hard_timings = timings
        return DeviceHardNegatives(d_mined, m)

    def _pairs_to_host(self, stage):
        """The sampled pairs' truth rows and targets (8 B per row of kinds 2 and 3)."""
        if not stage["n_selected"]:
            return np.zeros(0, np.int32), np.zeros(0, np.float32)
        return stage["d_pair_t"].to_host(), stage["d_target"].to_host()

    def _rows_and_split(self, stage, pair_t, target):
        """Fills `rows`; returns (every row's target, train rows, evaluation rows)."""
        import pandas as pd
        negative, positive, generated, selected = (stage[k] for k in ("negative", "positive", "generated", "selected"))
        sample_n = self.sample_n
        kind = np.concatenate((np.full(negative.shape[0] * sample_n, KIND_NEGATIVE, np.uint8),
                               np.full(positive.shape[0] * sample_n, KIND_POSITIVE, np.uint8),
                               np.full(generated.shape[0], KIND_GENERATED, np.uint8)))
        query_index = np.concatenate((np.repeat(selected, sample_n), generated.astype(np.int64)))
        truth_row = np.concatenate((pair_t.astype(np.int64), generated.astype(np.int64)))
        target = np.concatenate((target, np.ones(generated.shape[0], np.float32)))
        train_rows, evaluation_rows = evaluation_split(kind, self.seed, self.evaluation_fractions)
        evaluation = np.zeros(stage["n_rows"], dtype=bool)
        evaluation[evaluation_rows] = True
        self.rows = pd.DataFrame({"kind": kind, "query_index": query_index, "truth_row": truth_row, "target": target,
                                  "evaluation": evaluation})
        return target, train_rows, evaluation_rows

    def _device_stages(self, timings):
        """The stages both forms share, up to and including the features launches: every row's construct_features in
        one matrix in HBM."""
        started = time.perf_counter()
        device, k, sample_n = self.device, self.top_n, self.sample_n
        truth = self._truth_side(timings, started)
        n_truth = truth.table.n

        # ---- which train rows, in what order (kinds 2 and 3), and which truth rows are misspelled (kind 1)
        mark = time.perf_counter()
        negative, positive, selected, own, q_rowptr, q_cols, q_maxint, query_table = self._selected_queries()
        n_selected = selected.shape[0]
        truth_lengths = np.array([len(t) for t in self.truth_titles], dtype=np.int64)
        generated = np.nonzero(truth_lengths > GENERATED_MIN_LENGTH)[0].astype(np.int32)
        n_pairs = n_selected * sample_n
        n_rows = n_pairs + generated.shape[0]
        d_features = _lib.DeviceArray((max(n_rows, 1), FEATURES_COUNT), np.float32, device)
        timings["host_prepare"] += (time.perf_counter() - mark) * 1000.0

        # ---- top-n and the sample of every selected train row, one chunk of rows at a time
        timer = _lib.Timer(device)
        if n_selected:
            chunk = min(n_selected, self.chunk_queries or default_chunk(device, 4 * k + 64))
            d_rows = _lib.DeviceArray((chunk, k), np.int32, device)
            d_index = _lib.DeviceArray.from_host(selected.astype(np.int64), device)
            d_own = _lib.DeviceArray.from_host(own, device)
            d_pair_q = _lib.DeviceArray((n_pairs,), np.int32, device)
            d_pair_t = _lib.DeviceArray((n_pairs,), np.int32, device)
            d_target = _lib.DeviceArray((n_pairs,), np.float32, device)
            for first in range(0, n_selected, chunk):
                last = min(n_selected, first + chunk)
                rowptr, cols, maxint = slice_queries(q_rowptr, q_cols, q_maxint, first, last)
                d_rowptr = _lib.DeviceArray.from_host(rowptr, device)
                d_cols = _lib.DeviceArray.from_host(cols if cols.shape[0] else np.zeros(1, np.int32), device)
                d_maxint = _lib.DeviceArray.from_host(maxint, device)
                timer.start()
                truth.index.top_k_device(d_rowptr, d_cols, d_maxint, last - first, k, d_rows)
                timer.stop()
                truth.index.sync()
                timings["top_k"] += timer.elapsed_ms()
                timer.start()
                _lib.check(_lib.lib().ds_training_pairs_device(
                    d_rows.ptr, last - first, k, sample_n, ctypes.c_void_p(d_index.ptr.value + 8 * first),
                    ctypes.c_void_p(d_own.ptr.value + 4 * first), ctypes.c_uint64(self.seed), first, d_pair_q.ptr,
                    d_pair_t.ptr, d_target.ptr, None), "ds_training_pairs_device")
                timer.stop()
                timings["sample_pairs"] += timer.elapsed_ms()

        # ---- the misspelled truth titles, on the device
        misspelled = None
        if isinstance(self.misspelling_profile, str):          # "fit": learned once from the labelled train rows
            mark = time.perf_counter()
            self.misspelling_profile = validate_profile_argument(self.fit_misspelling_profile())
            timings["misspell_profile_fit"] = (time.perf_counter() - mark) * 1000.0
        if generated.shape[0]:
            mark = time.perf_counter()
            misspelled = misspell_table(truth.table, generated, self.seed, device, profile=self.misspelling_profile)
            timings["misspell" if self.misspelling_profile is None else "misspell_profile"] = \
                (time.perf_counter() - mark) * 1000.0

        # ---- construct_features of every row into one matrix: kinds 2 and 3 against the train titles, kind 1 against
        # the misspelled titles
        timer.start()
        if n_selected:
            _lib.check(_lib.lib().ds_construct_features_indexed_device(
                query_table.handle, truth.table.handle, d_pair_q.ptr, d_pair_t.ptr, 0, sample_n, SPACE_CODE, n_truth,
                n_pairs, d_features.ptr, None), "ds_construct_features_indexed_device")
        if misspelled is not None:
            d_gen_q = _lib.DeviceArray.from_host(np.arange(generated.shape[0], dtype=np.int32), device)
            d_gen_t = _lib.DeviceArray.from_host(generated, device)
            _lib.check(_lib.lib().ds_construct_features_indexed_device(
                misspelled.handle, truth.table.handle, d_gen_q.ptr, d_gen_t.ptr, 0, 1, SPACE_CODE, n_truth,
                generated.shape[0], ctypes.c_void_p(d_features.ptr.value + n_pairs * FEATURES_COUNT * 4), None),
                "ds_construct_features_indexed_device")
        timer.stop()
        timings["features"] = timer.elapsed_ms()

        return dict(d_features=d_features, n_rows=n_rows, n_selected=n_selected, negative=negative, positive=positive,
                    generated=generated, selected=selected, misspelled=misspelled,
                    d_pair_t=d_pair_t if n_selected else None, d_target=d_target if n_selected else None)
