"""Refreshing a model, the parts that need no GPU ("Refreshing a model"): the rule's identity on the
NumPy oracle alone (a model the oracle trainer grew, refreshed on its own data, comes back bit for bit; flipped labels
change it), node sums, gain and cover by hand, validate_refresh, and the declarations."""
import os
import re
import types

import numpy as np
import pytest

import forest_refresh_oracle as refreshed
import forest_train_oracle as oracle
from doppel_speller_amd import _lib
from doppel_speller_amd import forest as forest_module
from doppel_speller_amd.train import heap_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMETERS = dict(eta=0.1, reg_lambda=1.0, beta=5.0)


@pytest.fixture
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the library was called before the arguments were validated")
    monkeypatch.setattr(_lib, "lib", refuse)


def flat_arrays(trees, base_margin=0.0):
    """Per-tree dicts (ForestModel.from_trees' form) -> the flat arrays of a model, without the library."""
    offsets = np.zeros(len(trees) + 1, np.int64)
    offsets[1:] = np.cumsum([tree["feature"].shape[0] for tree in trees])
    dtypes = dict(feature=np.int32, threshold=np.float32, yes=np.int32, no=np.int32, missing=np.int32)
    out = {key: np.concatenate([tree[key] for tree in trees]).astype(dtype) for key, dtype in dtypes.items()}
    return dict(out, tree_offsets=offsets, base_margin=float(base_margin))


def oracle_model(x, y, rounds, max_depth):
    """The oracle trainer's trees as flat arrays, and its margins."""
    heaps, margins = oracle.train(x, y, rounds, max_depth=max_depth, **PARAMETERS)
    per_feature = oracle.cuts(x)
    offsets = np.zeros(len(per_feature) + 1, np.int32)
    offsets[1:] = np.cumsum([c.shape[0] for c in per_feature])
    cuts = np.concatenate(per_feature).astype(np.float32)
    trees = []
    for heap in heaps:
        info = np.stack([heap["state"], heap["feature"], heap["bin"], heap["default_left"]], axis=1)
        trees.append(heap_tree(info, heap["leaf"], cuts, offsets))
    return flat_arrays(trees), margins


@pytest.fixture(scope="module")
def grown():
    x, y = oracle.make_data(3000, 6, 11)
    arrays, margins = oracle_model(x, y, 8, 4)
    return x, y, arrays, margins


def test_a_model_refreshed_on_its_own_data_comes_back_bit_for_bit(grown):
    x, y, arrays, margins = grown
    out = refreshed.refresh(arrays, x, y, **PARAMETERS)
    leaves = arrays["feature"] < 0
    assert leaves.sum() > 60
    assert out["leaves"].tobytes() == arrays["threshold"].tobytes()
    assert out["margins"].tobytes() == margins.tobytes()
    assert out["empty_leaves"] == 0
    kept = refreshed.refresh(arrays, x, y, refresh_leaf=False, **PARAMETERS)
    assert kept["leaves"].tobytes() == arrays["threshold"].tobytes()
    assert np.array_equal(kept["node_sums"], out["node_sums"])


def test_flipped_labels_change_the_leaves_and_no_split(grown):
    x, y, arrays, _ = grown
    flipped = y.copy()
    rows = np.random.RandomState(3).choice(y.shape[0], 300, replace=False)
    flipped[rows] = 1 - flipped[rows]
    out = refreshed.refresh(arrays, x, flipped, **PARAMETERS)
    leaves = arrays["feature"] < 0
    changed = np.count_nonzero(out["leaves"][leaves] != arrays["threshold"][leaves])
    assert changed > leaves.sum() // 2
    assert out["leaves"][~leaves].tobytes() == arrays["threshold"][~leaves].tobytes()
    # another eta scales nothing but the leaves: the first tree's sums do not depend on it
    other = refreshed.refresh(arrays, x, flipped, eta=0.3, reg_lambda=1.0, beta=5.0)
    first = slice(0, int(arrays["tree_offsets"][1]))
    assert np.array_equal(other["node_sums"][first], out["node_sums"][first])
    assert not np.array_equal(other["node_sums"], out["node_sums"])


def test_an_inner_node_sums_its_children_and_a_root_all_rows(grown):
    x, y, arrays, _ = grown
    weights = np.random.RandomState(5).choice(np.array([0, 0.5, 1, 2], np.float32), y.shape[0])
    out = refreshed.refresh(arrays, x, y, weights=weights, **PARAMETERS)
    sums, offsets = out["node_sums"], arrays["tree_offsets"]
    for t in range(offsets.shape[0] - 1):
        begin = int(offsets[t])
        for i in range(begin, int(offsets[t + 1])):
            if arrays["feature"][i] >= 0:
                assert np.array_equal(sums[i], sums[begin + arrays["yes"][i]] + sums[begin + arrays["no"][i]])
        gh = refreshed.gradients(oracle.sigmoid32(out["before"][t]), y, 5.0, weights)
        assert np.array_equal(sums[begin], gh.sum(axis=0))


THREE = dict(feature=np.array([0, -1, -1], np.int32), threshold=np.array([0.5, -0.25, 0.75], np.float32),
             yes=np.array([1, 0, 0], np.int32), no=np.array([2, 0, 0], np.int32), missing=np.array([2, 0, 0], np.int32))


def test_gain_and_cover_of_a_three_node_tree_by_hand():
    arrays = flat_arrays([THREE])
    q = 1 << 30
    node_sums = np.array([[-2 * q, 6 * q], [-3 * q, 2 * q], [1 * q, 4 * q]], np.int64)
    gain = forest_module.split_gains(arrays, node_sums, 1.0)
    assert gain.tolist() == [9.0 / 3.0 + 1.0 / 5.0 - 4.0 / 7.0, 0.0, 0.0]
    model = types.SimpleNamespace(arrays=arrays, n_features=3)
    result = forest_module.RefreshResult(model, node_sums, 0, np.zeros(0, np.float32), 1.0, np.array([7, 4, ], np.int64))
    assert result.cover.tolist() == [6.0, 2.0, 4.0]
    assert result.gain.tolist() == gain.tolist()
    assert result.gain_importance().tolist() == [1.0, 0.0, 0.0]
    assert (result.initial_error, result.history, result.best_iteration) == (7, [4], 0)
    plain = forest_module.RefreshResult(model, node_sums, 2, np.zeros(0, np.float32), 1.0)
    assert (plain.initial_error, plain.history, plain.best_iteration, plain.empty_leaves) == (None, None, None, 2)
    # lambda 0 and a child without hessian: no evidence, no term
    empty = forest_module.split_gains(arrays, np.array([[q, q], [q, q], [0, 0]], np.int64), 0.0)
    assert empty.tolist() == [0.0, 0.0, 0.0]


def test_gain_importance_sums_per_feature_and_is_zero_without_gain():
    two = dict(THREE, feature=np.array([2, -1, -1], np.int32))
    arrays = flat_arrays([THREE, two, THREE])
    q = 1 << 30
    one = [[-2 * q, 6 * q], [-3 * q, 2 * q], [1 * q, 4 * q]]
    node_sums = np.array(one * 3, np.int64)
    model = types.SimpleNamespace(arrays=arrays, n_features=4)
    result = forest_module.RefreshResult(model, node_sums, 0, np.zeros(0, np.float32), 1.0)
    importance = result.gain_importance()
    assert importance.shape == (4,) and importance[1] == 0.0 and importance[3] == 0.0
    assert importance[0] == pytest.approx(2.0 / 3.0, rel=1e-15) and importance[2] == pytest.approx(1.0 / 3.0, rel=1e-15)
    none = forest_module.RefreshResult(model, np.zeros((9, 2), np.int64), 6, np.zeros(0, np.float32), 1.0)
    assert none.gain_importance().tolist() == [0.0] * 4


def test_the_oracle_keeps_a_leaf_without_evidence():
    """Rows of weight 0 on one side: that leaf keeps its value, is counted, and its sums are 0."""
    arrays = flat_arrays([THREE], base_margin=0.25)
    x = np.array([[0.0, 0, 0], [1.0, 0, 0], [np.nan, 0, 0], [0.25, 0, 0]], np.float32)
    y = np.array([1, 0, 1, 0], np.float32)
    weights = np.array([0, 1, 2, 0], np.float32)
    out = refreshed.refresh(arrays, x, y, weights=weights, **PARAMETERS)
    assert out["empty_leaves"] == 1 and out["node_sums"][1].tolist() == [0, 0]
    assert out["leaves"][1] == np.float32(-0.25) and out["leaves"][2] != np.float32(0.75)
    assert np.array_equal(out["node_sums"][0], out["node_sums"][2])
    assert out["before"][0].tolist() == [0.25] * 4


X, Y = np.zeros((4, 3), np.float32), np.array([0, 1, 0, 1], np.float32)
BAD = [
    (dict(features=np.zeros((4, 2))), "training features must be a"),
    (dict(features=np.zeros(3)), "training features must be a"),
    (dict(features=np.zeros((4, 3), dtype=object)), "must be numbers"),
    (dict(target=None), "target is missing"),
    (dict(target=Y[:3]), "labels"),
    (dict(target=np.array([0, 1, 2, 1])), "labels must all be 0 or 1"),
    (dict(target=np.array([0, 1, np.nan, 1])), "labels must all be 0 or 1"),
    (dict(eval_features=X), "go together"),
    (dict(eval_target=Y), "go together"),
    (dict(eval_features=np.zeros((4, 2)), eval_target=Y), "evaluation features must be a"),
    (dict(eval_features=np.zeros((0, 3)), eval_target=np.zeros(0)), "at least 1 row"),
    (dict(eval_features=X, eval_target=np.array([0, 1, 0, 3])), "evaluation labels must all be 0 or 1"),
    (dict(eta=0), "eta"), (dict(eta=-0.1), "eta"), (dict(eta=float("nan")), "eta"), (dict(eta="fast"), "eta"),
    (dict(reg_lambda=-1), "reg_lambda"), (dict(reg_lambda=float("inf")), "reg_lambda"),
    (dict(beta=0), "beta"), (dict(beta=-5), "beta"),
    (dict(sample_weight=np.ones(3)), "sample weights"),
    (dict(sample_weight=np.array([1, -1, 1, 1.0])), "negative"),
    (dict(sample_weight=np.array([1, np.nan, 1, 1.0])), "NaN"),
    (dict(sample_weight=np.zeros(4)), "total sample weight"),
    (dict(sample_weight=np.full(4, 2.0 ** 30)), "exceeds 2\\^32"),
    (dict(refresh_leaf=1), "refresh_leaf"), (dict(refresh_leaf=None), "refresh_leaf"),
]


def stub_model(n_features=3):
    """A ForestModel that never touched the library: what validation looks at."""
    class Stub(forest_module.ForestModel):
        def close(self):
            self.handle = None

    model = object.__new__(Stub)
    model.n_features, model.device, model.handle = n_features, 0, None
    return model


@pytest.mark.parametrize("arguments, message", BAD)
def test_validate_refresh_refuses_before_the_library(no_library, arguments, message):
    call = dict(dict(features=X, target=Y), **arguments)
    with pytest.raises(ValueError, match=message):
        forest_module.validate_refresh(3, **call)
    with pytest.raises(ValueError, match=message):
        stub_model().refresh(call.pop("features"), call.pop("target"), **call)


@pytest.mark.parametrize("arguments, message", [
    (dict(n=-1), "number of training rows"), (dict(n=True), "number of training rows"),
    (dict(n=2.0), "number of training rows"), (dict(n=1 << 31), "number of training rows"),
    (dict(n=3), "labels"),
    (dict(eval_target=Y, n_eval=0), "number of evaluation rows"),
    (dict(eval_target=Y, n_eval=3), "labels"),
    (dict(beta=2.0 ** 31), "exceeds 2\\^32"),
])
def test_validate_refresh_of_matrices_in_hbm(no_library, arguments, message):
    call = dict(dict(n=4, target=Y), **arguments)
    with pytest.raises(ValueError, match=message):
        forest_module.validate_refresh(3, None, call.pop("target"), None, call.pop("eval_target", None), **call)


def test_refresh_device_refuses_before_the_library(no_library):
    matrix = _lib.DeviceArray.view(4096, (4, 3), np.float32, 0)       # never read: the checks come first
    model = stub_model()
    for arguments, message in ((dict(d_eval_rows=matrix), "go together"), (dict(eval_target=Y), "go together"),
                               (dict(n=5, target=np.zeros(5)), "exceed the device matrix"),
                               (dict(d_rows=_lib.DeviceArray.view(4096, (4, 2), np.float32, 0)), r"float32\[n, 3\]"),
                               (dict(d_rows=None), "missing"), (dict(eta=0), "eta")):
        call = dict(dict(d_rows=matrix, n=4, target=Y), **arguments)
        with pytest.raises(ValueError, match=message):
            model.refresh_device(call.pop("d_rows"), call.pop("n"), call.pop("target"), **call)


def test_validate_refresh_cleans_its_arguments(no_library):
    v = forest_module.validate_refresh(3, X.astype(np.float64), [0, 1, 0, 1], X, Y, eta=np.float32(0.5), reg_lambda=0,
                                       beta=1, sample_weight=[1, 0, 2, 1])
    assert v["features"].dtype == np.float32 and v["target"].dtype == np.float32 and v["n"] == 4 and v["n_eval"] == 4
    assert v["sample_weight"].dtype == np.float32 and v["refresh_leaf"] is True
    assert (v["eta"], v["reg_lambda"], v["beta"]) == (0.5, 0.0, 1.0)
    none = forest_module.validate_refresh(3, np.zeros((0, 3)), np.zeros(0))
    assert none["n"] == 0 and none["eval_features"] is None and none["n_eval"] == 0
    hbm = forest_module.validate_refresh(3, None, Y, None, Y[:2], n=4, n_eval=2, refresh_leaf=np.bool_(False))
    assert hbm["features"] is None and hbm["n_eval"] == 2 and hbm["refresh_leaf"] is False


def test_refresh_model_validates_before_any_device_work(no_library):
    from doppel_speller_amd import train
    titles, ids = ["a title", "b title"], [1, 2]
    with pytest.raises(ValueError, match="must be a ForestModel"):
        train.refresh_model(titles, ids, titles, ids, object())
    with pytest.raises(ValueError, match="closed"):
        train.refresh_model(titles, ids, titles, ids, stub_model(66))
    model = stub_model(3)
    model.handle = 1
    with pytest.raises(ValueError, match="3 features"):
        train.refresh_model(titles, ids, titles, ids, model)
    model.n_features = 66
    with pytest.raises(ValueError, match="device"):
        train.refresh_model(titles, ids, titles, ids, model, device=1)
    with pytest.raises(ValueError, match="eta"):
        train.refresh_model(titles, ids, titles, ids, model, eta=0)
    with pytest.raises(ValueError, match="kind"):
        train.refresh_model(titles, ids, titles, ids, model, kind_weights={"unknown": 1.0})


def test_the_entries_are_declared_exported_and_built():
    import doppel_speller_amd as ds
    with open(os.path.join(ROOT, "include", "doppel_amd.h")) as handle:
        header = handle.read()
    for name in ("ds_forest_refresh", "ds_forest_refresh_device"):
        assert re.search(rf"^int {name}\(const ds_forest \*forest,", header, re.M), name
        assert name in _lib.EXPORTED_SYMBOLS
    assert len(set(_lib.EXPORTED_SYMBOLS)) == len(_lib.EXPORTED_SYMBOLS)
    assert "ds_refresh.hip" in _lib._SOURCES and len(set(_lib._SOURCES)) == len(_lib._SOURCES)
    assert "refresh_lds_nodes" in header
    for name in ("RefreshResult", "validate_refresh", "refresh_model", "split_gains"):
        assert hasattr(ds, name), name
    assert callable(ds.ForestModel.refresh) and callable(ds.ForestModel.refresh_device)
