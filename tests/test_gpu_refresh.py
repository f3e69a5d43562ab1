"""Refreshing a model on the GPU ("Refreshing a model"; csrc/ds_refresh.hip).  A model grown by
ForestTrainer and refreshed on its own data comes back bit for bit; everything else is compared, bit for bit, with the
NumPy restatement of tests/forest_refresh_oracle.py, which is handed the device's float32 probabilities (`trace`) as the
trainer's tests hand theirs.  The probabilities themselves are held to 2 ulp of NumPy's float32 sigmoid of the oracle's
margins on the changed-label runs, and to 4 ulp of the exactly rounded sigmoid everywhere (EXACT_STEPS below says why
and what was measured).  Not reachable on one GPU and through this ABI, and so not tested: a forest on another device, and a feature
count above the limit (ds_forest_create refuses it first)."""
import ctypes
import json
import math

import numpy as np
import pytest

import forest_refresh_oracle as refreshed
import forest_train_oracle as oracle
from forest_train_oracle import make_data

pytestmark = pytest.mark.gpu

PARAMETERS = dict(eta=0.1, reg_lambda=1.0, beta=5.0)
ROUNDS, DEPTH = 12, 4


def bits(a):
    return np.asarray(a).tobytes()


def ulps(a, b):
    """The largest distance, in float32 steps, between two arrays of positive float32 numbers."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    if a.size == 0:
        return 0
    return int(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max())


def grow(x, y, rounds=ROUNDS, depth=DEPTH, **more):
    """(model, the trainer's margins) after `rounds` steps."""
    import doppel_speller_amd as ds
    trainer = ds.ForestTrainer().begin(x, y, max_depth=depth, **PARAMETERS, **more)
    for _ in range(rounds):
        trainer.step()
    model, margins = trainer.model(), trainer.margins()
    trainer.close()
    return model, margins


@pytest.fixture(scope="module")
def data():
    x, y = make_data(3000, 6, 11)
    ex, ey = make_data(700, 6, 12)
    weights = np.random.RandomState(4).choice(np.array([0, 0, 0.5, 1, 3], np.float32), y.shape[0])
    flipped = y.copy()
    rows = np.random.RandomState(3).choice(y.shape[0], 300, replace=False)
    flipped[rows] = 1 - flipped[rows]
    return dict(x=x, y=y, ex=ex, ey=ey, weights=weights, flipped=flipped)


@pytest.fixture(scope="module")
def plain(data):
    return grow(data["x"], data["y"])


def exact_sigmoid32(margins):
    """The float32 nearest to the sigmoid of float32 margins, taken in float64."""
    with np.errstate(over="ignore"):
        return (1.0 / (1.0 + np.exp(-np.asarray(margins, dtype=np.float32).astype(np.float64)))).astype(np.float32)


# The device takes p = 1.0f / (1.0f + expf(-m)).  expf is within 1 ulp (the accuracy ROCm documents for it), the add and
# the correctly rounded divide add half an ulp each: a relative error of at most 2^-23 + 2^-24 + 2^-24 = 2^-22, which is
# at most 4 steps of a float32 (a step is at least 2^-24 of its number).  Every refresh of this file is held to that
# against the exactly rounded sigmoid.  NumPy's float32 exp has an error of its own, so the distance to sigmoid32 can be
# larger than the device's error; the issue's bound of 2 ulp against sigmoid32 is asserted where it was set, on the
# changed-label runs (numpy_steps=2), and printed everywhere.  Measured on an MI355X: 2 ulp from sigmoid32 on those runs;
# 3 ulp on three other runs of this file (257 rows, the 40-tree forest, refresh_leaf=False), where sigmoid32 itself is 2
# to 3 ulp from the exactly rounded sigmoid and the device 1 to 2 ("Refreshing a model").
EXACT_STEPS = 4


def against_oracle(model, x, y, weights=None, ex=None, ey=None, refresh_leaf=True, parameters=PARAMETERS,
                   numpy_steps=None):
    """One refresh with a trace, compared with the oracle in every output; returns (result, oracle's dict)."""
    result = model.refresh(x, y, ex, ey, sample_weight=weights, refresh_leaf=refresh_leaf, trace=True, **parameters)
    want = refreshed.refresh(model.arrays, x, y, result.trace, weights, refresh_leaf=refresh_leaf, eval_features=ex,
                             eval_target=ey, **parameters)
    got = result.model.arrays
    assert bits(got["threshold"]) == bits(want["leaves"])
    for key in ("feature", "yes", "no", "missing", "tree_offsets"):
        assert bits(got[key]) == bits(model.arrays[key])
    assert got["base_margin"] == model.arrays["base_margin"]
    assert np.array_equal(result.node_sums, want["node_sums"])
    assert bits(result.margins) == bits(want["margins"])
    assert result.empty_leaves == want["empty_leaves"]
    worst, exact = ulps(result.trace, oracle.sigmoid32(want["before"])), ulps(result.trace, exact_sigmoid32(want["before"]))
    print(f"trace over {result.trace.size} values: at most {worst} ulp from NumPy's float32 sigmoid, {exact} ulp from the "
          f"exactly rounded one (NumPy's own: {ulps(oracle.sigmoid32(want['before']), exact_sigmoid32(want['before']))})")
    assert exact <= EXACT_STEPS
    assert numpy_steps is None or worst <= numpy_steps
    if ex is not None:
        # no evaluation margin so close to the cut that 2 ulp of the sigmoid could move a row across it
        assert np.abs(want["eval_margins"].astype(np.float64) - math.log(9.0)).min() > 1e-5
        assert result.initial_error == want["initial_error"] and result.history == want["history"]
        assert result.best_iteration == int(np.argmin(want["history"])) if want["history"] else result.best_iteration is None
    else:
        assert result.history is None and result.initial_error is None and result.best_iteration is None
    return result, want


# ---- 1. the identity ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device_form", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_a_model_refreshed_on_its_own_data_comes_back_bit_for_bit(data, plain, weighted, device_form):
    from doppel_speller_amd import _lib
    x, y = data["x"], data["y"]
    weights = data["weights"] if weighted else None
    model, margins = grow(x, y, sample_weight=weights) if weighted else plain
    assert model.n_trees == ROUNDS and (model.arrays["feature"] < 0).sum() > 100
    if device_form:
        d_x = _lib.DeviceArray.from_host(x)
        result = model.refresh_device(d_x, x.shape[0], y, sample_weight=weights, **PARAMETERS)
        d_x.free()
    else:
        result = model.refresh(x, y, sample_weight=weights, **PARAMETERS)
    assert bits(result.model.arrays["threshold"]) == bits(model.arrays["threshold"])
    assert bits(result.margins) == bits(margins)
    # from the data: the leaves whose rows weigh nothing in all (the trainer's min_child_weight leaves none here)
    total = np.zeros(model.n_nodes)
    for t in range(model.n_trees):
        total += np.bincount(refreshed.walk(model.arrays, t, x), weights=weights, minlength=model.n_nodes)
    expected = int(np.count_nonzero(total[model.arrays["feature"] < 0] == 0))
    assert weights is None or (weights == 0).sum() > 500
    assert result.empty_leaves == expected == 0
    leaves = model.arrays["feature"] < 0
    assert (result.cover[leaves] >= 1.0).all() and result.gain[~leaves].min() > 0 and (result.gain[leaves] == 0).all()
    assert result.gain_importance().shape == model.feature_importance().shape
    assert result.gain_importance().sum() == pytest.approx(1.0)
    if weighted:
        model.close()
    result.model.close()


# ---- 2. against the oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parameters", [PARAMETERS, dict(eta=0.3, reg_lambda=0.0, beta=2.5),
                                        dict(eta=1.0, reg_lambda=7.5, beta=0.5)], ids=["same", "lambda0", "beta.5"])
def test_changed_labels_and_parameters_against_the_oracle(data, plain, parameters):
    model, _ = plain
    result, _ = against_oracle(model, data["x"], data["flipped"], data["weights"], data["ex"], data["ey"],
                               parameters=parameters, numpy_steps=2)
    leaves = model.arrays["feature"] < 0
    changed = np.count_nonzero(result.model.arrays["threshold"][leaves] != model.arrays["threshold"][leaves])
    assert changed > leaves.sum() // 2 and len(result.history) == model.n_trees
    result.model.close()


def test_the_device_form_with_an_evaluation_set_equals_the_host_form(data, plain):
    from doppel_speller_amd import _lib
    model, _ = plain
    host = model.refresh(data["x"], data["flipped"], data["ex"], data["ey"], sample_weight=data["weights"], **PARAMETERS)
    d_x, d_ex = _lib.DeviceArray.from_host(data["x"]), _lib.DeviceArray.from_host(data["ex"])
    device = model.refresh_device(d_x, 3000, data["flipped"], d_ex, 700, data["ey"], sample_weight=data["weights"],
                                  **PARAMETERS)
    fewer = model.refresh_device(d_x, 1000, data["flipped"][:1000], d_ex, 300, data["ey"][:300], **PARAMETERS)
    d_x.free()
    d_ex.free()
    assert bits(device.model.arrays["threshold"]) == bits(host.model.arrays["threshold"])
    assert np.array_equal(device.node_sums, host.node_sums) and bits(device.margins) == bits(host.margins)
    assert (device.history, device.initial_error, device.empty_leaves) == (host.history, host.initial_error,
                                                                          host.empty_leaves)
    first = model.refresh(data["x"][:1000], data["flipped"][:1000], data["ex"][:300], data["ey"][:300], **PARAMETERS)
    assert np.array_equal(fewer.node_sums, first.node_sums) and fewer.history == first.history
    for result in (host, device, fewer, first):
        result.model.close()


# ---- 3. edge shapes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_row_counts_around_a_wave_and_a_workgroup(data, plain, n):
    result, _ = against_oracle(plain[0], data["x"][:n], data["flipped"][:n], ex=data["ex"][:n], ey=data["ey"][:n])
    result.model.close()


def leaf_tree(value):
    return dict(feature=np.array([-1], np.int32), threshold=np.array([value], np.float32), yes=np.zeros(1, np.int32),
                no=np.zeros(1, np.int32), missing=np.zeros(1, np.int32))


def stump(feature, cut, low, high, missing_yes):
    return dict(feature=np.array([feature, -1, -1], np.int32), threshold=np.array([cut, low, high], np.float32),
                yes=np.array([1, 0, 0], np.int32), no=np.array([2, 0, 0], np.int32),
                missing=np.array([1 if missing_yes else 2, 0, 0], np.int32))


def test_a_single_leaf_first_and_trees_of_different_sizes(data, plain):
    import doppel_speller_amd as ds
    grown = ds.ForestModel.tree_list(plain[0].arrays)
    trees = [leaf_tree(0.5), grown[0], stump(0, 0.25, -0.5, 0.5, True), leaf_tree(-0.25), grown[5], grown[1]]
    model = ds.ForestModel.from_trees(trees, 6)
    assert len({tree["feature"].shape[0] for tree in trees}) >= 4
    result, want = against_oracle(model, data["x"], data["flipped"], data["weights"], data["ex"], data["ey"])
    assert result.empty_leaves == 0 and result.model.arrays["threshold"][0] != np.float32(0.5)
    assert result.node_sums[0, 1] > 0 and result.gain[0] == 0
    model.close()
    result.model.close()


def test_a_leaf_no_row_reaches_keeps_its_value_and_is_counted(data):
    import doppel_speller_amd as ds
    # nothing is below -inf, and column 0 holds no NaN: the `yes` leaves of trees 0 and 2 see no row
    trees = [stump(0, -np.inf, 0.75, -0.1, True), stump(1, 0.0, 0.2, -0.2, False), stump(0, -np.inf, -1.5, 0.1, True)]
    model = ds.ForestModel.from_trees(trees, 6)
    result, _ = against_oracle(model, data["x"], data["y"], ex=data["ex"], ey=data["ey"])
    assert result.empty_leaves == 2
    for node, value in ((1, 0.75), (7, -1.5)):
        assert result.model.arrays["threshold"][node] == np.float32(value)
        assert result.node_sums[node].tolist() == [0, 0] and result.cover[node] == 0
    assert np.array_equal(result.node_sums[0], result.node_sums[2])
    model.close()
    result.model.close()


def test_nan_features_follow_missing_on_either_side(data):
    import doppel_speller_amd as ds
    # column 2 is NaN in a fifth of the rows, column 4 in all of them
    trees = [stump(2, 0.0, 0.3, -0.3, True), stump(2, 0.0, 0.3, -0.3, False), stump(4, 0.0, 0.1, -0.1, True),
             stump(4, 0.0, 0.1, -0.1, False)]
    model = ds.ForestModel.from_trees(trees, 6)
    result, _ = against_oracle(model, data["x"], data["y"], data["weights"], data["ex"], data["ey"])
    missing = int(np.isnan(data["x"][:, 2]).sum())
    assert 0 < missing < 3000 and result.empty_leaves == 2
    assert result.node_sums[8].tolist() == [0, 0] and result.node_sums[10].tolist() == [0, 0]
    assert not np.array_equal(result.node_sums[1], result.node_sums[4])
    model.close()
    result.model.close()


def test_a_base_margin_that_is_not_zero(data):
    import doppel_speller_amd as ds
    def split(feature, cut, low, high, missing):
        return json.dumps({"nodeid": 0, "split": f"f{feature}", "split_condition": cut, "yes": 1, "no": 2,
                           "missing": missing, "children": [{"nodeid": 1, "leaf": low}, {"nodeid": 2, "leaf": high}]})
    model = ds.ForestModel.from_xgboost_dump([split(0, 0.5, -0.2, 0.4, 1), split(2, -0.25, 0.1, -0.3, 2),
                                              split(1, 1.0, -0.1, 0.2, 1)], 6, base_score=0.3)
    assert model.arrays["base_margin"] == math.log(0.3 / 0.7)
    result, want = against_oracle(model, data["x"], data["y"], ex=data["ex"], ey=data["ey"])
    assert bits(want["before"][0]) == bits(np.full(3000, np.float32(math.log(0.3 / 0.7)), np.float32))
    assert result.model.arrays["base_margin"] == model.arrays["base_margin"]
    model.close()
    result.model.close()


@pytest.fixture(scope="module")
def forty(data):
    model, margins = grow(data["x"][:1500], data["y"][:1500], rounds=40, depth=3)
    return model, margins


def test_forty_trees_in_sequence(data, forty):
    model, margins = forty
    same = model.refresh(data["x"][:1500], data["y"][:1500], **PARAMETERS)
    assert bits(same.model.arrays["threshold"]) == bits(model.arrays["threshold"]) and bits(same.margins) == bits(margins)
    result, _ = against_oracle(model, data["x"][:1500], data["flipped"][:1500], ex=data["ex"], ey=data["ey"])
    assert len(result.history) == 40
    same.model.close()
    result.model.close()


@pytest.fixture(scope="module")
def reference(data, plain):
    return plain[0].refresh(data["x"], data["flipped"], data["ex"], data["ey"], sample_weight=data["weights"],
                            **PARAMETERS)


def same_result(a, b):
    return bits(a.model.arrays["threshold"]) == bits(b.model.arrays["threshold"]) and \
        np.array_equal(a.node_sums, b.node_sums) and bits(a.margins) == bits(b.margins) and \
        (a.history, a.initial_error, a.empty_leaves) == (b.history, b.initial_error, b.empty_leaves)


@pytest.mark.parametrize("blocks", [1, 3])
def test_no_result_depends_on_the_grid(data, plain, reference, blocks):
    model = plain[0]
    model.option("max_blocks", blocks)
    try:
        capped = model.refresh(data["x"], data["flipped"], data["ex"], data["ey"], sample_weight=data["weights"],
                               **PARAMETERS)
    finally:
        model.option("max_blocks", 0)
    assert same_result(capped, reference)
    capped.model.close()


def test_the_lds_table_and_the_straight_adds_give_the_same_sums(data, plain, reference):
    model = plain[0]
    largest = int(np.diff(model.arrays["tree_offsets"]).max())
    try:
        for nodes in (largest, largest - 1, 1):       # all trees in LDS; the largest straight to HBM; all straight
            model.option("refresh_lds_nodes", nodes)
            other = model.refresh(data["x"], data["flipped"], data["ex"], data["ey"], sample_weight=data["weights"],
                                  **PARAMETERS)
            assert same_result(other, reference), nodes
            other.model.close()
    finally:
        model.option("refresh_lds_nodes", 0)
    from doppel_speller_amd import DoppelError
    for bad in (-1, 2049):
        with pytest.raises(DoppelError, match="refresh_lds_nodes"):
            model.option("refresh_lds_nodes", bad)


def test_weights_of_one_are_no_weights(data, plain):
    model = plain[0]
    ones = model.refresh(data["x"], data["flipped"], data["ex"], data["ey"], sample_weight=np.ones(3000), **PARAMETERS)
    none = model.refresh(data["x"], data["flipped"], data["ex"], data["ey"], **PARAMETERS)
    assert same_result(ones, none)
    ones.model.close()
    none.model.close()


def test_refresh_leaf_false_returns_the_old_leaves_and_the_first_trees_sums(data, plain, reference):
    model = plain[0]
    kept, _ = against_oracle(model, data["x"], data["flipped"], data["weights"], data["ex"], data["ey"],
                             refresh_leaf=False)
    assert bits(kept.model.arrays["threshold"]) == bits(model.arrays["threshold"])
    assert bits(kept.margins) == bits(model.predict(data["x"], output_margin=True))
    assert kept.history[-1] == kept.initial_error
    first = slice(0, int(model.arrays["tree_offsets"][1]))       # later trees see other margins once leaves change
    assert np.array_equal(kept.node_sums[first], reference.node_sums[first])
    # on the model's own data nothing changes either way: the same sums for every tree
    own = model.refresh(data["x"], data["y"], **PARAMETERS)
    own_kept = model.refresh(data["x"], data["y"], refresh_leaf=False, **PARAMETERS)
    assert np.array_equal(own.node_sums, own_kept.node_sums) and bits(own.margins) == bits(own_kept.margins)
    for result in (kept, own, own_kept):
        result.model.close()


def test_no_row_returns_the_model_unchanged(data, plain):
    model = plain[0]
    result, _ = against_oracle(model, np.zeros((0, 6), np.float32), np.zeros(0, np.float32))
    assert bits(result.model.arrays["threshold"]) == bits(model.arrays["threshold"])
    assert not result.node_sums.any() and result.margins.shape == (0,)
    assert result.empty_leaves == int((model.arrays["feature"] < 0).sum())
    with_eval, _ = against_oracle(model, np.zeros((0, 6), np.float32), np.zeros(0, np.float32), ex=data["ex"],
                                  ey=data["ey"])
    assert with_eval.history[-1] == with_eval.initial_error
    result.model.close()
    with_eval.model.close()


def test_a_model_without_trees(data):
    import doppel_speller_amd as ds
    model = ds.ForestModel.from_trees([], 6, base_margin=0.5)
    result, _ = against_oracle(model, data["x"][:100], data["y"][:100], ex=data["ex"], ey=data["ey"])
    assert result.history == [] and result.best_iteration is None and result.model.n_trees == 0
    assert bits(result.margins) == bits(np.full(100, 0.5, np.float32))
    model.close()
    result.model.close()


# ---- 4. the old model is unchanged --------------------------------------------------------------------------------------
def test_the_refreshed_model_is_new_and_the_old_one_untouched(data, plain):
    model = plain[0]
    fixed = data["ex"][:256]
    before, arrays = model.predict(fixed, output_margin=True), {k: np.copy(v) for k, v in model.arrays.items()}
    result = model.refresh(data["x"], data["flipped"], **PARAMETERS)
    assert bits(model.predict(fixed, output_margin=True)) == bits(before)
    for key, value in arrays.items():
        assert bits(model.arrays[key]) == bits(value)
    assert result.model is not model and result.model.handle.value != model.handle.value
    assert bits(result.model.predict(fixed, output_margin=True)) != bits(before)
    assert bits(result.model.predict(data["x"], output_margin=True)) == bits(result.margins)
    result.model.close()


# ---- 5. from raw titles ---------------------------------------------------------------------------------------------------
def test_refresh_model_from_raw_titles_equals_refresh_device_on_the_same_sets():
    import doppel_speller_amd as ds
    from doppel_speller_amd import synth
    w = synth.make_workload(800, 300, seed=31, query_seed=32)
    truth, train = synth._to_strings(w.t_flat, w.t_off), synth._to_strings(w.q_flat, w.q_off)
    ids = np.where(w.actual_row >= 0, w.title_id[np.maximum(w.actual_row, 0)], -1)
    sets_of = dict(top_n=10, sample_n=5, transform=False)
    trained = ds.train_model(truth, w.title_id, train, ids, seed=9, num_boost_round=6, early_stopping_rounds=6,
                             max_depth=3, **sets_of)
    model = trained.model
    weights = {"generated": 0.5, "positive": 2.0}
    parameters = dict(eta=0.2, reg_lambda=2.0, beta=5.0)
    result = ds.refresh_model(truth, w.title_id, train, ids, model, seed=10, kind_weights=weights, **sets_of, **parameters)
    fe = ds.FeatureEngineering(truth, w.title_id, train, ids, seed=10, **sets_of)
    sets = fe.generate_device_data_sets()
    assert sets.n_train > 300 and sets.n_evaluation > 0
    direct = model.refresh_device(sets.train, sets.n_train, sets.train_target, sets.evaluation, sets.n_evaluation,
                                  sets.evaluation_target, sample_weight=ds.kind_weights(fe.rows, weights), **parameters)
    sets.free()
    assert same_result(result, direct) and result.margins.shape == (sets.n_train,)
    assert len(result.history) == model.n_trees and result.initial_error is not None
    assert result.rows.equals(fe.rows)
    assert {"refresh", "total"} <= set(result.timings) and set(fe.timings) <= set(result.timings)
    assert all(value >= 0 for value in result.timings.values())
    assert result.gain_importance().shape == trained.feature_importance.shape
    for closing in (result.model, direct.model, model):
        closing.close()


# ---- 6. refusals through the ABI ----------------------------------------------------------------------------------------------
def abi_refresh(handle, x, y, weights=None, ex=None, ey=None, eta=0.1, reg_lambda=1.0, beta=5.0, refresh_leaf=1,
                n_nodes=0, outputs=True):
    from doppel_speller_amd import _lib
    p = _lib.pointer
    x, y = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32)
    leaves, sums = np.zeros(max(n_nodes, 1), np.float32), np.full((max(n_nodes, 1), 2), -7, np.int64)
    empty = ctypes.c_int64(-7)
    status = _lib.lib().ds_forest_refresh(
        handle, p(x), x.shape[0], p(y), p(weights), p(ex), p(ey), 0 if ex is None else ex.shape[0], eta, reg_lambda, beta,
        refresh_leaf, p(leaves if outputs else None), p(sums), None, None, ctypes.byref(empty), None)
    message = _lib.lib().ds_last_error().decode()
    assert (sums == -7).all() and empty.value == -7, "a refused call wrote its outputs"
    return status, message


X4 = np.zeros((4, 6), np.float32)
Y4 = np.array([0, 1, 0, 1], np.float32)
HUGE = np.full(4, 2.0 ** 30, np.float32)                       # 5 * 2^32 > 2^32 with four rows


@pytest.mark.parametrize("arguments, message", [
    (dict(y=[0, 1, 2, 1]), "labels: label 2 is not 0 or 1"),
    (dict(y=[0, np.nan, 0, 1]), "labels: label 1 is not 0 or 1"),
    (dict(ex=X4, ey=np.array([0, 1, 0, 0.5], np.float32)), "eval_labels: label 3 is not 0 or 1"),
    (dict(weights=np.array([1, -1, 1, 1], np.float32)), "weight 1 is negative"),
    (dict(weights=np.array([1, 1, np.nan, 1], np.float32)), "weight 2 is not finite"),
    (dict(weights=np.array([np.inf, 1, 1, 1], np.float32)), "weight 0 is not finite"),
    (dict(weights=HUGE), "exceeds 2\\^32"),
    (dict(weights=HUGE / 8, beta=40.0), "exceeds 2\\^32"),
    (dict(eta=0.0), "eta"), (dict(eta=-1.0), "eta"), (dict(eta=float("nan")), "eta"),
    (dict(reg_lambda=-0.5), "reg_lambda"), (dict(beta=0.0), "beta"), (dict(beta=-5.0), "beta"),
    (dict(refresh_leaf=2), "refresh_leaf"),
    (dict(ex=X4), "eval_features, eval_labels and n_eval"),
    (dict(outputs=False), "leaf_out"),
])
def test_the_abi_refuses_by_name(plain, arguments, message):
    model = plain[0]
    call = dict(dict(x=X4, y=Y4, n_nodes=model.n_nodes), **arguments)
    status, text = abi_refresh(model.handle, call.pop("x"), call.pop("y"), **call)
    assert status == -1 and text.startswith("ds_forest_refresh: ")
    import re
    assert re.search(message, text), text


def test_the_abi_refuses_a_null_forest_and_a_tree_that_is_no_binary_tree():
    import doppel_speller_amd as ds
    status, text = abi_refresh(None, X4, Y4)
    assert status == -1 and "forest is null" in text
    crooked = stump(0, 0.5, -0.1, 0.1, True)
    crooked["no"] = np.array([1, 0, 0], np.int32)                  # both branches lead to node 1
    model = ds.ForestModel.from_trees([stump(1, 0.0, 0.2, -0.2, False), crooked], 6)
    status, text = abi_refresh(model.handle, X4, Y4, n_nodes=6)
    assert status == -1 and "node 0 of tree 1 is no binary split" in text
    model.close()


def test_the_guards_edge_is_legal(data):
    """max(beta, 1) * the total weight = 2^32 exactly: accepted, and the sums are those of the oracle."""
    import doppel_speller_amd as ds
    model = ds.ForestModel.from_trees([stump(0, 0.0, 0.2, -0.2, False)], 6)
    weights = np.full(4, 2.0 ** 30, np.float32)
    result, _ = against_oracle(model, data["x"][:4], Y4, weights, parameters=dict(eta=0.1, reg_lambda=1.0, beta=1.0))
    assert result.node_sums[0, 1] > 2 ** 57
    model.close()
    result.model.close()
