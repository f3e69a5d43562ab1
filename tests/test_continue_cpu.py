"""Continuing from a model ("Continuing from a model") without a GPU: validate_init_model, the
array forms of ForestModel.head / extended, the oracle's own k + m identity (tests/forest_continue_oracle.py), and
assertions from the inputs alone that the data of tests/test_gpu_continue.py reaches what those tests rely on."""
import ctypes
import os

import numpy as np
import pytest

import forest_continue_oracle as continued
import forest_train_oracle as oracle
from forest_train_oracle import make_data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the base shape of the GPU tests: 2,500 training rows (no multiple of 256), 700 evaluation rows, 7 features
BASE = dict(n=2500, n_eval=700, nf=7, seed=91, eval_seed=92, other_seed=95)
BASE_PARAMETERS = dict(max_depth=4, eta=0.3)
K, M = 5, 4
# early stopping: (training seed, evaluation seed, early_stopping_rounds) at eta 1.0
STOPPING = {"minimum_inside": (97, 98, 4), "initial_is_lower": (91, 92, 3)}
STOPPING_PARAMETERS = dict(max_depth=4, eta=1.0)


def base_data():
    x, y = make_data(BASE["n"], BASE["nf"], BASE["seed"])
    ex, ey = make_data(BASE["n_eval"], BASE["nf"], BASE["eval_seed"])
    return x, y, ex, ey


def between_cuts_forest(features, seed=5):
    """A hand-built forest every threshold of which lies strictly between two neighbouring cuts of `features` (or
    beyond the last one): midpoints of the sorted distinct values of its column."""
    trees = continued.random_forest(6, 3, features.shape[1], seed)
    rng = np.random.RandomState(seed + 1)
    for tree in trees:
        for i in np.nonzero(tree["feature"] >= 0)[0]:
            column = features[:, tree["feature"][i]]
            values = np.unique(column[np.isfinite(column)])
            if values.size < 2:
                tree["threshold"][i] = np.float32(0.25)
                continue
            at = rng.randint(0, values.size - 1)
            tree["threshold"][i] = np.float32((np.float64(values[at]) + np.float64(values[at + 1])) / 2)
    return trees


def stub_model(n_features=7, base_margin=0.0, device=0, handle=True):
    """A ForestModel that never touched the library: what validate_init_model looks at."""
    import doppel_speller_amd as ds

    class Stub(ds.ForestModel):
        def close(self):                # nothing of the library's to give back
            self.handle = None

    model = object.__new__(Stub)
    model.arrays = dict(continued.flat_forest([]), base_margin=float(base_margin))
    model.n_features, model.n_trees, model.device, model.cover = n_features, 0, device, None
    model.handle = ctypes.c_void_p(1) if handle else None
    return model


# ---- validate_init_model ------------------------------------------------------------------------------------------------
def test_validate_init_model_refusals():
    import doppel_speller_amd as ds
    from doppel_speller_amd import train
    assert ds.validate_init_model is train.validate_init_model
    good = stub_model()
    assert ds.validate_init_model(good, 7) is good and ds.validate_init_model(good, 7, device=0) is good
    with pytest.raises(ValueError, match="must be a ForestModel"):
        ds.validate_init_model({"feature": []}, 7)
    with pytest.raises(ValueError, match="must be a ForestModel"):
        ds.validate_init_model(None, 7)
    with pytest.raises(ValueError, match="has 7 features, the training features 8"):
        ds.validate_init_model(good, 8)
    with pytest.raises(ValueError, match="base margin"):
        ds.validate_init_model(stub_model(base_margin=0.5), 7)
    with pytest.raises(ValueError, match="device 1"):
        ds.validate_init_model(good, 7, device=1)
    with pytest.raises(ValueError, match="closed"):
        ds.validate_init_model(stub_model(handle=False), 7)
    # an xgboost import with the default base_score has base margin log(0.5 / 0.5) = 0 and qualifies; 0.3 does not
    assert ds.ForestModel.parse_xgboost_dump([], base_score=0.5)["base_margin"] == 0.0
    assert ds.ForestModel.parse_xgboost_dump([], base_score=0.3)["base_margin"] != 0.0


def test_every_entry_validates_before_any_device_work():
    """A bad init_model is a ValueError of fit, fit_device's checks, cross_validate, train_model and
    tune_model_parameters on a machine without a GPU: nothing was created before the check."""
    import doppel_speller_amd as ds
    x, y = make_data(50, 7, 1)
    wrong = stub_model(n_features=8)
    with pytest.raises(ValueError, match="8 features"):
        ds.ForestTrainer().fit(x, y, init_model=wrong)
    with pytest.raises(ValueError, match="8 features"):
        ds.ForestTrainer().begin(x, y, init_model=wrong)
    with pytest.raises(ValueError, match="8 features"):
        ds.ForestTrainerBatch().begin(x, y, np.arange(50) % 2, [dict(held_out=0)], init_model=wrong)
    with pytest.raises(ValueError, match="8 features"):
        ds.cross_validate(x, y, dict(max_depth=2), n_folds=2, init_model=wrong)
    titles = ["alpha beta", "gamma delta"]
    with pytest.raises(ValueError, match="7 features, the training features 66"):
        ds.train_model(titles, [1, 2], titles, [1, 2], init_model=stub_model())
    with pytest.raises(ValueError, match="7 features, the training features 66"):
        ds.tune_model_parameters(titles, [1, 2], titles, [1, 2], dict(max_depth=2), n_folds=2, init_model=stub_model())
    with pytest.raises(ValueError, match="must be a ForestModel"):
        ds.train_model(titles, [1, 2], titles, [1, 2], init_model="model.npz")


# ---- head / extended ----------------------------------------------------------------------------------------------------
def same_arrays(a, b):
    return all(a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes()
               for key in continued.TREE_KEYS + ("tree_offsets",)) and a["base_margin"] == b["base_margin"]


def test_head_and_extended_round_trip():
    import doppel_speller_amd as ds
    trees = continued.random_forest(5, 2, 7, 3) + continued.random_forest(2, 4, 7, 4)
    whole = continued.flat_forest(trees)
    model = ds.ForestModel
    assert same_arrays(model.head_arrays(whole, 7), whole)
    empty = model.head_arrays(whole, 0)
    assert empty["tree_offsets"].tolist() == [0] and all(empty[key].shape == (0,) for key in continued.TREE_KEYS)
    for k in (0, 1, 5, 7):
        head = model.head_arrays(whole, k)
        assert same_arrays(head, continued.flat_forest(trees[:k]))
        assert same_arrays(model.extended_arrays(head, trees[k:]), whole)
        assert same_arrays(model.extended_arrays(head, model.tree_list(whole)[k:]), whole)
    assert same_arrays(model.extended_arrays(whole, []), whole)
    assert [tree["feature"].shape[0] for tree in model.tree_list(whole)] == [7] * 5 + [31] * 2
    for bad in (-1, 8, 2.0, True, None):
        with pytest.raises(ValueError, match="n_trees"):
            model.head_arrays(whole, bad)
    head = model.head_arrays(whole, 3)
    head["threshold"][0] = 99.0                      # a copy: the source is untouched
    assert whole["threshold"][0] != 99.0


# ---- the oracle's own identity ------------------------------------------------------------------------------------------
SAMPLED = dict(subsample=0.5, colsample_bytree=0.6, colsample_bylevel=0.5, sample_seed=17)


@pytest.mark.parametrize("extra", [{}, dict(subsample=0.5), SAMPLED], ids=["plain", "rows", "all"])
def test_oracle_k_plus_m_equals_k_then_m(extra):
    x, y, ex, ey = base_data()
    parameters = dict(BASE_PARAMETERS, **extra)
    straight = continued.train(x, y, K + M, None, ex, ey, **parameters)
    first = continued.train(x, y, K, None, ex, ey, **parameters)
    init = continued.flat_forest(first["flat"])
    second = continued.train(x, y, M, init, ex, ey, **parameters)
    assert first["initial_error"] == continued.error_of(np.zeros(BASE["n_eval"], np.float32), ey)
    for a, b in zip(straight["trees"], first["trees"] + second["trees"]):
        assert all(a[key].tobytes() == b[key].tobytes() for key in a)
    assert same_arrays(continued.flat_forest(straight["flat"]), continued.flat_forest(first["flat"] + second["flat"]))
    assert straight["margins"].tobytes() == second["margins"].tobytes()
    assert straight["eval_margins"].tobytes() == second["eval_margins"].tobytes()
    assert straight["errors"][K:] == second["errors"] and second["initial_error"] == straight["errors"][K - 1]
    # the seed is the walk of the RAW features: it lands on the margins the bins gave
    assert continued.leaf_sums(init, x).tobytes() == first["margins"].tobytes()
    if extra:       # numbered from 0 again, the new trees differ: the identity does test the tree number
        restarted = continued.ContinueBooster(x, y, init, parameters)
        restarted.first_tree = 0
        for _ in range(M):
            restarted.step()
        assert restarted.margins().tobytes() != straight["margins"].tobytes()


# ---- what the GPU tests' data reaches, from the inputs alone -----------------------------------------------------------
def test_base_data_walks_nan_and_negative_zero():
    x, y, ex, ey = base_data()
    assert np.isnan(x[:, 2]).any() and np.isnan(ex[:, 2]).any() and np.isnan(x[:, 4]).all()
    assert (np.signbit(x[:, 5]) & (x[:, 5] == 0)).any()                   # -0.0
    trees = between_cuts_forest(x)
    per_feature = oracle.cuts(x)
    inner = [(int(f), t) for tree in trees for f, t in zip(tree["feature"], tree["threshold"]) if f >= 0]
    assert all(t not in per_feature[f] for f, t in inner) and len(inner) == 6 * 7
    assert len({f for f, _ in inner}) >= 5
    events = {}
    continued.leaf_sums(continued.flat_forest(trees), x, events)
    assert events["nan"] > 100 and events["yes"] > 100 and events["no"] > 100
    # a threshold of exactly 0.0 on the column of +-0.0: -0.0 goes to `no`, as +0.0 does
    zero = dict(feature=np.array([5, -1, -1], np.int32), threshold=np.array([0.0, 1.0, 2.0], np.float32),
                yes=np.array([1, 0, 0], np.int32), no=np.array([2, 0, 0], np.int32),
                missing=np.array([1, 0, 0], np.int32))
    sums = continued.leaf_sums(continued.flat_forest([zero]), x)
    assert (sums[x[:, 5] == 0] == 2.0).all() and (sums[x[:, 5] == -np.inf] == 1.0).all()


def test_new_data_has_other_cuts_than_the_init_models():
    """The init model of the new-data test comes from matrix A; matrix B has other cuts, so thresholds of A's trees are
    not among them (with NumPy's sigmoid standing in for the device's when A's trees are grown)."""
    x, y, _, _ = base_data()
    other, _ = make_data(BASE["n"], BASE["nf"], BASE["other_seed"])
    first = continued.train(x, y, K, None, **BASE_PARAMETERS)
    cuts_b = oracle.cuts(other)
    thresholds = [(int(f), t) for tree in first["flat"] for f, t in zip(tree["feature"], tree["threshold"]) if f >= 0]
    outside = [(f, t) for f, t in thresholds if t not in cuts_b[f]]
    assert len(outside) >= 10 and len(thresholds) >= K
    assert continued.leaf_sums(continued.flat_forest(first["flat"]), other).std() > 0


@pytest.mark.parametrize("case", sorted(STOPPING))
def test_early_stopping_data_has_its_minimum_inside(case):
    seed, eval_seed, patience = STOPPING[case]
    x, y = make_data(BASE["n"], BASE["nf"], seed)
    ex, ey = make_data(BASE["n_eval"], BASE["nf"], eval_seed)
    run = continued.train(x, y, K + 10, None, ex, ey, **STOPPING_PARAMETERS)
    new, initial = run["errors"][K:], run["errors"][K - 1]
    stop = next(r for r in range(len(new)) if r - int(np.argmin(new[:r + 1])) >= patience)
    best = int(np.argmin(new[:stop + 1]))               # the first minimum of the rounds looked at
    assert best < stop < len(new) - 1                   # stops early, and not on its last round
    if case == "initial_is_lower":
        assert initial < min(new) and best == 0         # as a candidate the init model would win: it is none
    else:
        assert best >= 2 and new[best] < initial


# ---- the C ABI's refusals that need no device --------------------------------------------------------------------------
def test_seed_entries_refuse_null_handles_without_a_device():
    import doppel_speller_amd as ds
    from doppel_speller_amd import _lib
    library = ctypes.CDLL(ds.build_library())
    library.ds_last_error.restype = ctypes.c_char_p
    assert library.ds_trainer_seed(None, None, None, None, None) == -1
    assert b"ds_trainer_seed: trainer is null" in library.ds_last_error()
    assert library.ds_trainer_seed_device(None, None, None, None, None, None) == -1
    assert b"ds_trainer_seed_device: trainer is null" in library.ds_last_error()
    assert library.ds_trainer_batch_seed(None, None, None, None) == -1
    assert b"ds_trainer_batch_seed: batch is null" in library.ds_last_error()
    assert library.ds_trainer_batch_seed_device(None, None, None, None, None) == -1
    assert b"ds_trainer_batch_seed_device: batch is null" in library.ds_last_error()
    assert {"ds_trainer_seed", "ds_trainer_seed_device", "ds_trainer_batch_seed",
            "ds_trainer_batch_seed_device"} <= set(_lib.EXPORTED_SYMBOLS)
    with open(os.path.join(ROOT, "include", "doppel_amd.h")) as handle:
        header = " ".join(handle.read().split())
    assert ("int ds_trainer_seed(ds_trainer *trainer, const ds_forest *forest, const float *features, "
            "const float *eval_features, int64_t *initial_error);") in header
