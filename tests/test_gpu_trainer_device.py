"""The trainer fed from HBM (ForestTrainer.begin_device / fit_device, ds_gather_rows_device) against the host-fed trainer
and the NumPy restatement of its contract (tests/forest_train_oracle.py), bit for bit."""
import ctypes

import numpy as np
import pytest

import forest_train_oracle as oracle
from forest_train_oracle import make_data
from test_gpu_trainer import check_rounds, crafted_early_stopping_set

pytestmark = pytest.mark.gpu
MODEL_KEYS = ("feature", "threshold", "yes", "no", "missing", "tree_offsets")


def upload(array):
    from doppel_speller_amd import _lib
    return _lib.DeviceArray.from_host(np.ascontiguousarray(array, dtype=np.float32))


def test_begin_device_bins_equal_begin_and_the_oracle():
    import doppel_speller_amd as ds
    x, y = make_data(5003, 66, 1)
    x[:, 10] = np.random.RandomState(2).randint(0, 255, x.shape[0])     # exactly 255 distinct values
    x[:, 11] = np.random.RandomState(3).randint(0, 256, x.shape[0])     # 256: quantile cuts
    host = ds.ForestTrainer().begin(x, y)
    d_x = upload(x)
    device = ds.ForestTrainer().begin_device(d_x, x.shape[0], y)
    d_x.free()                                                          # the trainer keeps no pointer to the matrix
    assert device.cuts.tobytes() == host.cuts.tobytes() and device.cut_offsets.tolist() == host.cut_offsets.tolist()
    assert np.array_equal(device.bins(), host.bins())
    assert np.array_equal(device.bins(), oracle.bins(x, oracle.cuts(x)))
    for max_bin in (16, 2):
        d_x = upload(x)
        assert np.array_equal(ds.ForestTrainer().begin_device(d_x, x.shape[0], y, max_bin=max_bin).bins(),
                              ds.ForestTrainer().begin(x, y, max_bin=max_bin).bins())


@pytest.mark.parametrize("n,nf,depth,lam,mcw,eta", [(1000, 66, 5, 1.0, 1.0, 0.1), (20000, 10, 6, 0.5, 2.0, 0.2),
                                                    (100000, 66, 5, 1.0, 1.0, 0.1)])
def test_trees_margins_and_errors_of_a_device_fed_trainer_match_the_oracle(n, nf, depth, lam, mcw, eta):
    import doppel_speller_amd as ds
    x, y = make_data(n, nf, n + depth)
    ex, ey = make_data(max(1, n // 3), nf, n + depth + 1)
    d_x, d_ex = upload(x), upload(ex)
    trainer = ds.ForestTrainer().begin_device(d_x, n, y, d_ex, ex.shape[0], ey, max_depth=depth, eta=eta,
                                              min_child_weight=mcw, reg_lambda=lam)
    d_x.free()
    d_ex.free()
    trees = check_rounds(trainer, x, y, ex, ey, 30, depth, eta, mcw, lam)
    split_rounds = sum(int(np.count_nonzero(tree["state"] != oracle.ABSENT)) > 1 for tree in trees)
    assert split_rounds == 30


def test_device_matrix_by_address_with_n_features():
    import doppel_speller_amd as ds
    x, y = make_data(3000, 20, 4)
    d_x = upload(x)
    by_address = ds.ForestTrainer().begin_device(d_x.ptr.value, 3000, y, n_features=20)
    assert np.array_equal(by_address.bins(), ds.ForestTrainer().begin(x, y).bins())


@pytest.mark.parametrize("patience", [10, 150])
def test_fit_device_stops_where_fit_stops(patience):
    """patience 10 stops early; 150 runs every round and keeps the first minimum of the whole history, which lies
    inside it (tests/test_gpu_trainer.py asserts that of this set)."""
    import doppel_speller_amd as ds
    x, y, ex, ey = crafted_early_stopping_set()
    host = ds.ForestTrainer()
    host_model = host.fit(x, y, ex, ey, max_depth=2, early_stopping_rounds=patience, num_boost_round=150)
    device = ds.ForestTrainer()
    device_model = device.fit_device(upload(x), x.shape[0], y, upload(ex), ex.shape[0], ey, max_depth=2,
                                     early_stopping_rounds=patience, num_boost_round=150)
    if patience == 10:
        assert len(host.trees) < 150 and host.best_iteration == len(host.trees) - 1 - patience
    else:
        assert len(host.trees) == 150 and 0 < host.best_iteration < 149
    assert device.best_iteration == host.best_iteration and device.history == host.history
    assert len(device.trees) == len(host.trees)
    assert device_model.n_trees == host_model.n_trees == host.best_iteration + 1
    for key in MODEL_KEYS:
        assert device_model.arrays[key].tobytes() == host_model.arrays[key].tobytes(), key


def test_fit_device_without_an_evaluation_set_keeps_every_round():
    import doppel_speller_amd as ds
    x, y = make_data(30000, 66, 8)
    host = ds.ForestTrainer()
    host_model = host.fit(x, y, num_boost_round=12)
    device = ds.ForestTrainer()
    device_model = device.fit_device(upload(x), x.shape[0], y, num_boost_round=12)
    assert device.best_iteration == host.best_iteration == 11 and device.history == [None] * 12
    for key in MODEL_KEYS:
        assert device_model.arrays[key].tobytes() == host_model.arrays[key].tobytes(), key
    assert np.array_equal(device.margins().view(np.uint32), host.margins().view(np.uint32))


def small_sets():
    """300 training rows x 5 features and 100 evaluation rows: more than one block of rows, no multiple of a block."""
    return make_data(300, 5, 21) + make_data(100, 5, 22)


@pytest.mark.parametrize("every_branch", [False, True], ids=["plain", "metrics_sampling_init_model"])
def test_fit_and_fit_device_leave_the_same_trainer_behind(every_branch):
    """The second case takes every optional branch of begin on both forms: metrics, subsampling, an init model."""
    import doppel_speller_amd as ds
    x, y, ex, ey = small_sets()
    parameters = dict(max_depth=2, num_boost_round=3)
    if every_branch:
        init = ds.ForestTrainer().fit(x, y, max_depth=2, num_boost_round=2)
        assert init.n_trees == 2
        parameters.update(eval_metrics=("auc", "logloss"), subsample=0.5, init_model=init)
    host, device = ds.ForestTrainer(), ds.ForestTrainer()
    host.fit(x, y, ex, ey, **parameters)
    device.fit_device(upload(x), 300, y, upload(ex), 100, ey, **parameters)
    for name in ("n", "n_features", "n_eval", "params", "history", "best_iteration", "initial_error", "eval_metrics"):
        assert getattr(device, name) == getattr(host, name), name
    assert (host.n, host.n_features, host.n_eval, len(host.history), len(host.trees)) == (300, 5, 100, 3, 3)
    assert device.cuts.tobytes() == host.cuts.tobytes() and device.cut_offsets.tolist() == host.cut_offsets.tolist()
    assert list(device.metrics_history) == list(host.metrics_history) and len(device.trees) == len(host.trees)
    assert {"cuts", "bin"} <= set(device.timings)
    if every_branch:
        assert host.eval_metrics == ("auc", "logloss") and isinstance(host.initial_error, int)
        assert sorted(host.metrics_history) == ["evaluation-auc", "evaluation-logloss", "train-auc", "train-logloss"]
        assert host.params["subsample"] == 0.5 and 2 <= host.best_iteration <= 4
    else:
        assert host.eval_metrics == () and host.metrics_history == {} and host.initial_error is None


def test_a_refused_second_begin_leaves_the_trainer_stepping():
    """A begin that is refused has touched nothing: the next step is the next round of the first begin."""
    import doppel_speller_amd as ds
    x, y, ex, ey = small_sets()
    trainer, twin = (ds.ForestTrainer().begin(x, y, ex, ey, max_depth=2) for _ in range(2))
    assert trainer.step() == twin.step()
    handle = trainer.handle
    with pytest.raises(ValueError, match="max_depth"):
        trainer.begin(x, y, ex, ey, max_depth=9)
    with pytest.raises(ValueError, match="max_depth"):
        trainer.begin_device(upload(x), 300, y, max_depth=9)
    assert trainer.handle is handle and len(trainer.trees) == 1 and trainer.params["max_depth"] == 2
    assert trainer.step() == twin.step() and trainer.history == twin.history and len(trainer.trees) == 2
    assert all(np.array_equal(trainer.trees[1][key], twin.trees[1][key]) for key in twin.trees[1])
    assert np.array_equal(trainer.margins().view(np.uint32), twin.margins().view(np.uint32))


def gather(source, rows, n_src=None, sentinel=-5.0):
    """(status, destination on the host with one sentinel row before and after)."""
    from doppel_speller_amd import _lib
    source = np.ascontiguousarray(source, dtype=np.float32)
    nf = source.shape[1]
    rows = np.asarray(rows, dtype=np.int64)
    d_source = _lib.DeviceArray.from_host(source)
    d_rows = _lib.DeviceArray.from_host(rows if rows.shape[0] else np.zeros(1, np.int64))
    d_out = _lib.DeviceArray.from_host(np.full((rows.shape[0] + 2, nf), sentinel, np.float32))
    status = _lib.lib().ds_gather_rows_device(d_source.ptr, nf, d_rows.ptr, rows.shape[0],
                                              source.shape[0] if n_src is None else n_src,
                                              ctypes.c_void_p(d_out.ptr.value + 4 * nf), None)
    return status, d_out.to_host()


@pytest.mark.parametrize("nf", [1, 7, 66, 96])
def test_gather_rows_equals_fancy_indexing(nf):
    rng = np.random.RandomState(nf)
    source, _ = make_data(5000, nf, nf)                                  # NaNs, infinities and signed zeros travel as bits
    for rows in (rng.permutation(5000), rng.randint(0, 5000, 12345), np.arange(5000), np.array([4999]),
                 np.repeat(np.array([17, 3]), 700), np.zeros(0, np.int64)):
        status, out = gather(source, rows)
        assert status == 0
        assert np.array_equal(out[1:-1].view(np.uint32), source[rows].view(np.uint32))
        assert (out[0] == -5.0).all() and (out[-1] == -5.0).all()


def test_gather_rows_refuses_an_index_out_of_range_and_writes_nothing():
    from doppel_speller_amd import _lib
    source, _ = make_data(1000, 12, 2)
    for bad in (1000, -1, 2 ** 40, -2 ** 40):
        rows = np.arange(300, dtype=np.int64)
        rows[137] = bad
        status, out = gather(source, rows)
        assert status == -1 and b"out of range" in _lib.lib().ds_last_error()
        assert (out == -5.0).all()
    status, out = gather(source, [0, 999, 500], n_src=500)              # n_src is the bound, not the allocation
    assert status == -1 and (out == -5.0).all()
    status, out = gather(source, [0, 499], n_src=500)
    assert status == 0 and np.array_equal(out[1:-1].view(np.uint32), source[[0, 499]].view(np.uint32))
