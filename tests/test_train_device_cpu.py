"""The one-call train-model step without a GPU: the new C entry points (ds_feature_cuts_device, ds_cuts_option,
ds_trainer_create_device, ds_trainer_set_eval_device, ds_gather_rows_device) refuse bad arguments with DS_E_ARG and a
message before they touch a device; train_model and fit_device refuse what validate_training and validate_fit refuse
before the library is loaded; and the crafted cut-test columns reach both branches of the cut rule and its boundaries."""
import ctypes
import inspect

import numpy as np
import pytest

import cuts_cases
import forest_train_oracle as oracle
from doppel_speller_amd import _lib


@pytest.fixture
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the library was called before the arguments were validated")
    monkeypatch.setattr(_lib, "lib", refuse)


@pytest.fixture(scope="module")
def library():
    import doppel_speller_amd as ds
    handle = ctypes.CDLL(ds.build_library())
    handle.ds_last_error.restype = ctypes.c_char_p
    return handle


def _p(array):
    return array.ctypes.data_as(ctypes.c_void_p)


def test_feature_cuts_device_argument_errors(library):
    matrix = np.zeros((4, 3), np.float32)          # never read: every call fails before the device is touched
    cuts, offsets = np.full(3 * 254, -7, np.float32), np.full(4, -7, np.int32)

    def call(features=_p(matrix), n=4, nf=3, max_bin=256, cuts_=_p(cuts), offsets_=_p(offsets)):
        return library.ds_feature_cuts_device(features, ctypes.c_int64(n), nf, max_bin, cuts_, offsets_, 0, None)

    for kwargs in (dict(features=None), dict(cuts_=None), dict(offsets_=None)):
        assert call(**kwargs) == -1 and b"null pointer" in library.ds_last_error()
    for n in (0, -1, 2 ** 31):
        assert call(n=n) == -1 and b"rows out of range [1, 2^31)" in library.ds_last_error()
    for nf in (0, 97):
        assert call(nf=nf) == -1 and b"n_features" in library.ds_last_error()
    for max_bin in (1, 257):
        assert call(max_bin=max_bin) == -1 and b"max_bin" in library.ds_last_error()
    assert (cuts == -7).all() and (offsets == -7).all()
    assert library.ds_cuts_option(None, ctypes.c_int64(1)) == -1 and b"null name" in library.ds_last_error()
    assert library.ds_cuts_option(b"column_groups", ctypes.c_int64(1)) == -1
    assert b"unknown option" in library.ds_last_error()
    for value in (-1, 97):
        assert library.ds_cuts_option(b"column_group", ctypes.c_int64(value)) == -1
        assert b"column_group" in library.ds_last_error()


def test_trainer_create_device_argument_errors(library):
    d = ctypes.c_double
    matrix = np.zeros((4, 2), np.float32)
    cuts, offsets = np.array([0.5, 1.5], np.float32), np.array([0, 1, 2], np.int32)
    out = ctypes.c_void_p(1)

    def call(features=_p(matrix), n=4, nf=2, cuts_=_p(cuts), offsets_=_p(offsets), depth=5, out_=ctypes.byref(out)):
        return library.ds_trainer_create_device(features, ctypes.c_int64(n), ctypes.c_int32(nf), cuts_, offsets_, depth,
                                                d(0.1), d(1), d(1), d(5), 0, out_)

    assert call(out_=None) == -1 and b"ds_trainer_create_device: out is null" in library.ds_last_error()
    for kwargs in (dict(features=None), dict(cuts_=None), dict(offsets_=None)):
        assert call(**kwargs) == -1 and b"ds_trainer_create_device: null input" in library.ds_last_error()
        assert not out.value
    for n in (0, 2 ** 31):
        assert call(n=n) == -1 and b"rows out of range" in library.ds_last_error()
    for nf in (0, 97):
        assert call(nf=nf) == -1 and b"n_features" in library.ds_last_error()
    assert call(depth=9) == -1 and b"max_depth" in library.ds_last_error()
    descending = np.array([1.5, 0.5], np.float32)
    one_feature = np.array([0, 2, 2], np.int32)
    assert call(cuts_=_p(descending), offsets_=_p(one_feature)) == -1
    assert b"strictly ascending" in library.ds_last_error()
    labels = np.zeros(4, np.float32)
    assert library.ds_trainer_set_eval_device(None, _p(matrix), _p(labels), ctypes.c_int64(4)) == -1
    assert b"ds_trainer_set_eval_device: null argument" in library.ds_last_error()


def test_gather_rows_device_argument_errors(library):
    buffer = np.zeros(64, np.int64)

    def call(src=_p(buffer), nf=2, rows=_p(buffer), n_rows=3, n_src=8, dst=_p(buffer)):
        return library.ds_gather_rows_device(src, nf, rows, ctypes.c_int64(n_rows), ctypes.c_int64(n_src), dst, None)

    for kwargs in (dict(src=None), dict(rows=None), dict(dst=None)):
        assert call(**kwargs) == -1 and b"null pointer" in library.ds_last_error()
    for nf in (0, 97):
        assert call(nf=nf) == -1 and b"n_features" in library.ds_last_error()
    assert call(n_rows=-1) == -1 and b"n_rows = -1" in library.ds_last_error()
    assert call(n_rows=2 ** 31) == -1 and b"n_rows" in library.ds_last_error()
    for n_src in (0, 2 ** 31):
        assert call(n_src=n_src) == -1 and b"n_src" in library.ds_last_error()
    assert call(src=None, rows=None, dst=None, n_rows=0) == 0          # an empty list touches nothing
    assert not buffer.any()


GOOD = dict(truth_titles=["alpha beta", "gamma delta", "epsilon zeta"], truth_title_ids=[5, 6, 7],
            train_titles=["alpha bet", "unknown"], train_title_ids=[5, -1], top_n=2, sample_n=1)


@pytest.mark.parametrize("change, message", [
    (dict(train_title_ids=[5]), "train title ids"),
    (dict(train_title_ids=[5, 99]), "not truth title ids"),
    (dict(train_title_ids=[5, -2]), "truth title ids or -1"),
    (dict(sample_n=3), "exceeds top_n"),
    (dict(sample_n=0), "sample_n"),
    (dict(seed=-1), "seed"),
    (dict(truth_title_ids=[5, 5, 7]), ""),
    (dict(top_n=4), ""),
    (dict(evaluation_fractions={"negative": 1.0}), "evaluation fraction"),
    (dict(evaluation_fractions={"neutral": 0.1}), "unknown evaluation fractions"),
    (dict(max_depth=9), "max_depth"),
    (dict(eta=0), "eta"),
    (dict(num_boost_round=0), "num_boost_round"),
    (dict(early_stopping_rounds=True), "early_stopping_rounds"),
    (dict(max_bin=1), "max_bin"),
    (dict(reg_lambda=0, min_child_weight=0), "cannot both be 0"),
    (dict(beta=float("nan")), "beta"),
    (dict(depth=3), "unknown fit parameters"),
])
def test_train_model_validates_before_the_library(no_library, change, message):
    import doppel_speller_amd as ds
    with pytest.raises(ValueError, match=message):
        ds.train_model(**dict(GOOD, **change))


class _Matrix:
    """Stands in for a DeviceArray of a given shape: validation looks at nothing else."""

    def __init__(self, rows, columns):
        self.shape = (rows, columns)


@pytest.mark.parametrize("arguments, message", [
    (dict(d_features=None), "missing"),
    (dict(d_features=_Matrix(4, 97)), "97 columns"),
    (dict(d_features=1234), "n_features is needed"),
    (dict(n=0), "training rows"),
    (dict(n=2 ** 31), "training rows"),
    (dict(target=np.zeros(3)), "4 training rows but 3 labels"),
    (dict(target=np.array([0, 1, 2, 0])), "labels must all be 0 or 1"),
    (dict(d_eval_features=_Matrix(2, 3)), "go together"),
    (dict(eval_target=np.zeros(2)), "go together"),
    (dict(d_eval_features=_Matrix(2, 4), n_eval=2, eval_target=np.zeros(2)), "4 columns, training features 3"),
    (dict(d_eval_features=_Matrix(2, 3), n_eval=0, eval_target=np.zeros(0)), "evaluation rows"),
    (dict(d_eval_features=_Matrix(2, 3), n_eval=2, eval_target=np.array([0.5, 1])), "evaluation labels"),
    (dict(max_depth=0), "max_depth"),
    (dict(eta=-1), "eta"),
    (dict(min_child_weight=0, reg_lambda=0), "cannot both be 0"),
    (dict(max_bin=257), "max_bin"),
    (dict(num_boost_round=0), "num_boost_round"),
    (dict(early_stopping_rounds=0), "early_stopping_rounds"),
])
def test_fit_device_validates_before_the_library(no_library, arguments, message):
    import doppel_speller_amd as ds
    call = dict(dict(d_features=_Matrix(4, 3), n=4, target=np.array([0, 1, 0, 1])), **arguments)
    with pytest.raises(ValueError, match=message):
        ds.ForestTrainer().fit_device(**call)
    begin = {k: v for k, v in call.items() if k not in ("num_boost_round", "early_stopping_rounds")}
    if begin == call:
        with pytest.raises(ValueError, match=message):
            ds.ForestTrainer().begin_device(**begin)


def test_fit_device_rejects_what_validate_fit_rejects(no_library):
    """The same parameter sets fail on both paths with the same message."""
    import doppel_speller_amd as ds
    from doppel_speller_amd.train import validate_fit, validate_fit_device
    x, y = np.zeros((4, 3), np.float32), np.array([0, 1, 0, 1])
    for parameters in (dict(max_depth=9), dict(eta=float("inf")), dict(beta=0), dict(max_bin=True),
                       dict(reg_lambda=-1), dict(min_child_weight="x"), dict(num_boost_round=1.5)):
        with pytest.raises(ValueError) as host:
            validate_fit(x, y, **parameters)
        with pytest.raises(ValueError) as device:
            validate_fit_device(_Matrix(4, 3), 4, y, **parameters)
        assert str(host.value) == str(device.value)
    assert validate_fit_device(_Matrix(4, 3), 4, y)[5] == validate_fit(x, y)[4]
    assert ds.compute_cuts_device is not None


LEGAL = dict(num_boost_round=7, early_stopping_rounds=3, max_depth=3, eta=0.3, min_child_weight=2.0, reg_lambda=0.5,
             beta=2.0, max_bin=16, subsample=0.5, colsample_bytree=0.6, colsample_bylevel=0.7, sample_seed=9,
             eval_metrics=("auc",))
ROUNDS = ("num_boost_round", "early_stopping_rounds")
X4, Y4 = np.zeros((4, 3), np.float32), np.array([0, 1, 0, 1])


def test_every_parameter_name_is_taken_by_keyword_at_every_entry(no_library):
    """Each name of validate_parameters' signature, at a legal value that is not its default, alone and all together:
    the validate_* return it, the trainer's forms get past their checks to the library (the fixture's refusal)."""
    import doppel_speller_amd as ds
    from doppel_speller_amd.train import validate_fit, validate_fit_device, validate_parameters
    names = list(inspect.signature(validate_parameters).parameters)
    assert sorted(names) == sorted(LEGAL)
    defaults = validate_parameters()
    for given in [{name: LEGAL[name]} for name in names] + [LEGAL]:
        assert all(defaults[name] != value for name, value in given.items())
        for params in (validate_parameters(**given), validate_fit(X4, Y4, **given)[4],
                       validate_fit_device(_Matrix(4, 3), 4, Y4, **given)[5]):
            assert params == dict(defaults, **given)
        calls = [lambda: ds.ForestTrainer().fit(X4, Y4, **given),
                 lambda: ds.ForestTrainer().fit_device(_Matrix(4, 3), 4, Y4, **given)]
        stepped = {name: value for name, value in given.items() if name not in ROUNDS}
        if stepped:
            calls += [lambda: ds.ForestTrainer().begin(X4, Y4, **stepped),
                      lambda: ds.ForestTrainer().begin_device(_Matrix(4, 3), 4, Y4, **stepped)]
        for call in calls:
            with pytest.raises(AssertionError, match="before the arguments were validated"):
                call()


def test_the_step_forms_do_not_know_the_round_names(no_library):
    import doppel_speller_amd as ds
    with pytest.raises(TypeError, match="num_boost_round"):
        ds.ForestTrainer().begin(X4, Y4, num_boost_round=3)
    with pytest.raises(TypeError, match="early_stopping_rounds"):
        ds.ForestTrainer().begin_device(_Matrix(4, 3), 4, Y4, early_stopping_rounds=3)


def test_a_refused_second_begin_keeps_the_first_state(no_library):
    import doppel_speller_amd as ds
    trainer = ds.ForestTrainer()
    handle, trees, params = ctypes.c_void_p(1), [object()], dict(max_depth=2)      # stand-ins for a begun trainer's
    trainer.handle, trainer.trees, trainer.params = handle, trees, params
    try:
        for again in (lambda: trainer.begin(X4, Y4, max_depth=9), lambda: trainer.fit(X4, Y4, max_depth=9),
                      lambda: trainer.begin_device(_Matrix(4, 3), 4, Y4, max_depth=9),
                      lambda: trainer.fit_device(_Matrix(4, 3), 4, Y4, max_depth=9)):
            with pytest.raises(ValueError, match="max_depth"):
                again()
            assert trainer.handle is handle and trainer.trees is trees and trainer.params is params
    finally:
        trainer.handle = None                      # the stand-in is nothing the library could give back


def test_compute_cuts_device_validates_before_the_library(no_library):
    import doppel_speller_amd as ds
    for arguments, message in (((None, 4), "missing"), ((_Matrix(4, 3), 0), "n must be"), ((1234, 4), "n_features"),
                               ((_Matrix(4, 3), 2 ** 31), "n must be")):
        with pytest.raises(ValueError, match=message):
            ds.compute_cuts_device(*arguments)
    with pytest.raises(ValueError, match="max_bin"):
        ds.compute_cuts_device(_Matrix(4, 3), 4, max_bin=1)


def _distinct(column):
    present = column[column == column]
    return np.unique(np.where(present == 0, np.float32(0.0), present))


@pytest.mark.parametrize("max_bin", [256, 16, 2])
def test_crafted_columns_reach_both_branches_and_the_boundaries(max_bin):
    """With d distinct values a column takes the distinct branch (d - 1 cuts: all but the smallest) up to d = max_bin
    - 1 and the quantile branch (at most max_bin - 2 picks, so never all d - 1) from d = max_bin on."""
    columns = cuts_cases.crafted_columns()
    for count in (max_bin - 2, max_bin - 1, max_bin):
        column = columns["all_nan"] if count == 0 else columns[f"distinct_{count}"]
        distinct = _distinct(column)
        assert distinct.shape[0] == count
        cuts = oracle.cuts_of(column, max_bin)
        if count <= max_bin - 1:
            assert cuts_cases.same_bits(cuts, distinct[1:].astype(np.float32))
        else:
            assert cuts.shape[0] <= max_bin - 2 < distinct[1:].shape[0]
            assert np.isin(cuts, distinct[1:]).all() and (np.diff(cuts) > 0).all()
    branches = {name: _distinct(column).shape[0] <= max_bin - 1 for name, column in columns.items()}
    assert any(branches.values()) and not all(branches.values())


def test_crafted_columns_hold_what_they_are_named_for():
    columns = cuts_cases.crafted_columns()
    matrix, names = cuts_cases.crafted_matrix()
    assert matrix.shape == (cuts_cases.ROWS, len(names)) and len(names) <= 96
    assert np.isnan(columns["all_nan"]).all() and np.count_nonzero(~np.isnan(columns["one_value"])) == 1
    zeros = columns["signed_zeros"]
    assert np.count_nonzero(np.signbit(zeros) & (zeros == 0)) and np.count_nonzero(~np.signbit(zeros) & (zeros == 0))
    assert oracle.cuts_of(zeros).tolist() == [0.0, 1.0]                 # -0.0 and +0.0 are one value
    assert np.isposinf(columns["infinities"]).any() and np.isneginf(columns["infinities"]).any()
    bits = columns["denormals"].view(np.uint32)
    assert ((bits & 0x7f800000) == 0).all() and (bits >> 31).any() and not (bits >> 31).all()
    assert _distinct(columns["denormals_few"]).shape[0] == 6          # the two zeros are one, no flush to zero
    for name in ("shared_low_positive", "shared_low_mixed"):
        assert (columns[name].view(np.uint32) & 0xffff == 0x1234).all() and np.isfinite(columns[name]).all()
    assert (columns["shared_low_positive"] > 0).all()
    mixed = columns["shared_low_mixed"]
    assert (mixed > 0).any() and (mixed < 0).any()
    share = np.mean(np.isnan(columns["nan_30"]))
    assert 0.25 < share < 0.35
    assert _distinct(columns["distinct_255_nan_30"]).shape[0] == 255
