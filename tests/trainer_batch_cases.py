"""The argument errors of ds_trainer_batch_create(_device) through ctypes: every limit of the header violated in turn.
The entries refuse before they touch a device, so tests/test_tuning_cpu.py runs the cases, on every machine."""
import ctypes

import numpy as np


def _p(array):
    return array.ctypes.data_as(ctypes.c_void_p)


def batch_create_cases():
    """(keyword changes of a good ds_trainer_batch_create call, what ds_last_error must name): every limit of the
    header violated in turn."""
    default = [5, 0.1, 1, 1, 5]
    with_params = lambda *values: np.array([default, list(values)], np.float64)
    return [
        (dict(features=None), "features is null"), (dict(cuts=None), "cuts is null"), (dict(offsets=None), "cut_offsets is null"),
        (dict(labels=None), "labels is null"), (dict(fold=None), "fold is null"), (dict(params=None), "params is null"),
        (dict(held_out=None), "held_out is null"),
        (dict(n=0), "n = 0"), (dict(n=2 ** 31), "n = 2147483648"),
        (dict(nf=0), "n_features = 0"), (dict(nf=97), "n_features = 97"),
        (dict(n_models=0), "n_models = 0"), (dict(n_models=257), "n_models = 257"),
        (dict(n_folds=0), "n_folds = 0"), (dict(n_folds=256), "n_folds = 256"),
        (dict(fold=np.array([0, 1, 2, 3], np.uint8)), "fold[3] = 3"),
        (dict(held_out=np.array([0, 3], np.int32)), "held_out[1] = 3"),
        (dict(held_out=np.array([-2, 0], np.int32)), "held_out[0] = -2"),
        (dict(params=with_params(0, 0.1, 1, 1, 5)), "max_depth"), (dict(params=with_params(9, 0.1, 1, 1, 5)), "max_depth"),
        (dict(params=with_params(2.5, 0.1, 1, 1, 5)), "max_depth"),
        (dict(params=with_params(5, 0, 1, 1, 5)), "params of model 1: eta"),
        (dict(params=with_params(5, 0.1, -1, 1, 5)), "params of model 1"),
        (dict(params=with_params(5, 0.1, 0, 0, 5)), "not both 0"),
        (dict(params=with_params(5, 0.1, 1, 1, float("nan"))), "params of model 1"),
        (dict(labels=np.array([0, 1, 0.5, 1], np.float32)), "labels: label 2"),
        (dict(cuts=np.array([1.5, 0.5], np.float32), offsets=np.array([0, 2, 2], np.int32)), "strictly ascending"),
    ]


def call_batch_create(library, entry, **changes):
    arrays = dict(features=np.zeros((4, 2), np.float32), cuts=np.array([0.5, 1.5], np.float32),
                  offsets=np.array([0, 1, 2], np.int32), labels=np.array([0, 1, 0, 1], np.float32),
                  fold=np.array([0, 1, 2, 0], np.uint8), params=np.array([[5, 0.1, 1, 1, 5]] * 2, np.float64),
                  held_out=np.array([0, -1], np.int32))
    scalars = dict(n=4, nf=2, n_folds=3, n_models=2)
    for key, value in changes.items():
        (arrays if key in arrays else scalars)[key] = value
    pointer = {key: None if value is None else _p(value) for key, value in arrays.items()}
    out = ctypes.c_void_p(1)
    status = getattr(library, entry)(pointer["features"], ctypes.c_int64(scalars["n"]), ctypes.c_int32(scalars["nf"]),
                                     pointer["cuts"], pointer["offsets"], pointer["labels"], pointer["fold"],
                                     ctypes.c_int32(scalars["n_folds"]), ctypes.c_int32(scalars["n_models"]),
                                     pointer["params"], pointer["held_out"], 0, ctypes.byref(out))
    return status, out.value, library.ds_last_error().decode()
