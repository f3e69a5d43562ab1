"""Monotone constraints without a GPU ("Monotone constraints"): every refusal of
validate_monotone_constraints, the call order of every entry (a bad vector is refused before the library is reached and a
refused begin keeps the trainer's state), the NumPy restatement's own properties on the cases the GPU tests use (the
constraints reject candidates, change every tree, clamp leaves and leave no violation, while the unconstrained trees have
some), ForestModel's violation count on hand-built trees and the C ABI's two new entries."""
import ctypes
import os
import re

import numpy as np
import pytest

import forest_monotone_oracle as monotone_oracle
import forest_train_oracle as oracle
from doppel_speller_amd import _lib
from doppel_speller_amd.forest import ForestModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X4, Y4 = np.zeros((4, 3), np.float32), np.array([0, 1, 0, 1])
NAMES = ("alpha", "beta", "gamma")


@pytest.fixture
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the library was called before the arguments were validated")
    monkeypatch.setattr(_lib, "lib", refuse)


class _Matrix:
    """Stands in for a DeviceArray of a given shape: validation looks at nothing else."""

    def __init__(self, rows, columns):
        self.shape = (rows, columns)


# ---- validate_monotone_constraints --------------------------------------------------------------------------------------
@pytest.mark.parametrize("constraints, message", [
    ([1, 0], "3 features but 2 monotone_constraints"),
    ([1, 0, 0, -1], "3 features but 4 monotone_constraints"),
    (np.zeros((3, 1), np.int8), "1-D"),
    (1, "1-D sequence of 3 signs or a dict"),
    ("+0-", "1-D sequence of 3 signs or a dict"),
    ([True, False, False], "entry 0 must be -1, 0 or 1, not True"),
    (np.array([False, True, False]), "must hold -1, 0 or 1, not bool"),
    (np.array(["1", "0", "0"]), "must hold -1, 0 or 1, not"),
    ([0, 0.5, 0], "entry 1 must be -1, 0 or 1, not 0.5"),
    ([0, 0, float("nan")], "entry 2 must be -1, 0 or 1, not nan"),
    (np.array([0, np.nan, 0]), "entry 1 must be -1, 0 or 1"),
    ([0, 2, 0], "entry 1 must be -1, 0 or 1, not 2"),
    ([0, -2, 0], "entry 1 must be -1, 0 or 1, not -2"),
    ([0, "1", 0], "entry 1 must be -1, 0 or 1, not '1'"),
    ([0, None, 0], "entry 1 must be -1, 0 or 1, not None"),
    (dict(delta=1), r"names unknown features \['delta'\]"),
    (dict(alpha=1, delta=1, epsilon=-1), r"names unknown features \['delta', 'epsilon'\]"),
    (dict(alpha=2), "the sign of 'alpha' must be -1, 0 or 1, not 2"),
    (dict(alpha=True), "the sign of 'alpha' must be -1, 0 or 1, not True"),
    (dict(beta=0.5), "the sign of 'beta' must be -1, 0 or 1, not 0.5"),
])
def test_validate_monotone_constraints_refuses(constraints, message):
    import doppel_speller_amd as ds
    with pytest.raises(ValueError, match=message):
        ds.validate_monotone_constraints(constraints, 3, NAMES)


def test_a_dict_needs_the_feature_names_and_as_many_as_features():
    import doppel_speller_amd as ds
    with pytest.raises(ValueError, match="needs the feature names"):
        ds.validate_monotone_constraints(dict(alpha=1), 3)
    with pytest.raises(ValueError, match="2 feature names for 3 features"):
        ds.validate_monotone_constraints(dict(alpha=1), 3, NAMES[:2])


def test_validate_monotone_constraints_returns_contiguous_int8():
    import doppel_speller_amd as ds
    for given in ([1, 0, -1], (1.0, 0.0, -1.0), np.array([1, 0, -1], np.int64), np.arange(6)[::2] // 2 * 0 + [1, 0, -1],
                  np.array([1.0, 0.0, -1.0], np.float32), dict(alpha=1, gamma=-1), dict(gamma=-1.0, alpha=np.int8(1))):
        out = ds.validate_monotone_constraints(given, 3, NAMES)
        assert out.dtype == np.int8 and out.shape == (3,) and out.flags["C_CONTIGUOUS"]
        assert out.tolist() == [1, 0, -1]
    assert ds.validate_monotone_constraints({}, 3, NAMES).tolist() == [0, 0, 0]
    assert ds.validate_monotone_constraints([0, 0, 0], 3).tolist() == [0, 0, 0]


def test_ratio_constraints_name_the_seventeen_ratio_columns():
    import doppel_speller_amd as ds
    assert len(ds.RATIO_FEATURE_NAMES) == 17 and set(ds.RATIO_FEATURE_NAMES) < set(ds.FEATURE_NAMES)
    assert ds.RATIO_FEATURE_NAMES[:2] == ("title_ratio", "rebuilt_title_ratio")
    assert ds.RATIO_FEATURE_NAMES[2:] == tuple(f"word_{k}_best_ratio" for k in range(1, 16))
    constraints = ds.ratio_constraints()
    assert constraints == {name: 1 for name in ds.RATIO_FEATURE_NAMES}
    vector = ds.validate_monotone_constraints(constraints, ds.FEATURES_COUNT, ds.FEATURE_NAMES)
    assert vector.sum() == 17 and [ds.FEATURE_NAMES[f] for f in np.nonzero(vector)[0]] == list(ds.RATIO_FEATURE_NAMES)
    constraints["title_ratio"] = 0                      # a fresh dict every call
    assert ds.ratio_constraints()["title_ratio"] == 1


# ---- call order -----------------------------------------------------------------------------------------------------
BAD = [([1, 0], "3 features but 2"), ([0, 2, 0], "entry 1"), ([True, 0, 0], "not True"), ([0.5, 0, 0], "not 0.5"),
       ([0, float("nan"), 0], "not nan"), ("abc", "1-D sequence"), (dict(alpha=1), "needs the feature names")]
FOLD = np.array([0, 1, 0, 1])


def _entries(constraints):
    import doppel_speller_amd as ds
    return [lambda: ds.ForestTrainer().begin(X4, Y4, monotone_constraints=constraints),
            lambda: ds.ForestTrainer().fit(X4, Y4, monotone_constraints=constraints, num_boost_round=2),
            lambda: ds.ForestTrainer().begin_device(_Matrix(4, 3), 4, Y4, monotone_constraints=constraints),
            lambda: ds.ForestTrainer().fit_device(_Matrix(4, 3), 4, Y4, monotone_constraints=constraints),
            lambda: ds.ForestTrainerBatch().begin(X4, Y4, FOLD, [dict(held_out=0)], monotone_constraints=constraints),
            lambda: ds.ForestTrainerBatch().begin_device(_Matrix(4, 3), 4, Y4, FOLD, [dict(held_out=0)],
                                                         monotone_constraints=constraints),
            lambda: ds.cross_validate(X4, Y4, dict(max_depth=2), n_folds=2, monotone_constraints=constraints)]


@pytest.mark.parametrize("constraints, message", BAD)
def test_a_bad_vector_is_refused_before_the_library(no_library, constraints, message):
    for call in _entries(constraints):
        with pytest.raises(ValueError, match=message):
            call()


@pytest.mark.parametrize("constraints", [[1, 0, -1], [0, 0, 0], np.array([0, 1, 0], np.int8)])
def test_a_legal_vector_reaches_the_library_at_every_entry(no_library, constraints):
    import doppel_speller_amd as ds
    for call in _entries(constraints):
        with pytest.raises(AssertionError, match="before the arguments were validated"):
            call()
    assert ds.ForestTrainer().monotone_constraints is None and ds.ForestTrainerBatch().monotone_constraints is None
    with pytest.raises(TypeError):
        ds.ForestTrainer().fit(X4, Y4, None, None, constraints)          # by keyword only


def test_train_model_and_tuning_validate_before_the_library(no_library):
    import doppel_speller_amd as ds
    good = dict(truth_titles=["alpha beta", "gamma delta", "epsilon zeta"], truth_title_ids=[5, 6, 7],
                train_titles=["alpha bet", "unknown"], train_title_ids=[5, -1], top_n=2, sample_n=1)
    for constraints, message in ((dict(title_ration=1), r"unknown features \['title_ration'\]"),
                                 (dict(title_ratio=3), "the sign of 'title_ratio'"), ([1, 0, 0], "66 features but 3"),
                                 ([0.5] * 66, "entry 0")):
        with pytest.raises(ValueError, match=message):
            ds.train_model(**good, monotone_constraints=constraints)
        with pytest.raises(ValueError, match=message):
            ds.tune_model_parameters(**good, parameters=dict(max_depth=2), n_folds=2, monotone_constraints=constraints)


def test_a_refused_second_begin_keeps_the_first_state(no_library):
    import doppel_speller_amd as ds
    trainer = ds.ForestTrainer()
    handle, trees, params, kept = ctypes.c_void_p(1), [object()], dict(max_depth=2), np.ones(3, np.int8)
    trainer.handle, trainer.trees, trainer.params, trainer.monotone_constraints = handle, trees, params, kept
    bad = [0, 2, 0]
    try:
        for again in (lambda: trainer.begin(X4, Y4, monotone_constraints=bad),
                      lambda: trainer.fit(X4, Y4, monotone_constraints=bad),
                      lambda: trainer.begin_device(_Matrix(4, 3), 4, Y4, monotone_constraints=bad),
                      lambda: trainer.fit_device(_Matrix(4, 3), 4, Y4, monotone_constraints=bad)):
            with pytest.raises(ValueError, match="entry 1"):
                again()
            assert trainer.handle is handle and trainer.trees is trees and trainer.params is params
            assert trainer.monotone_constraints is kept
    finally:
        trainer.handle = None                      # the stand-in is nothing the library could give back
    batch = ds.ForestTrainerBatch()
    batch.handle, batch.trees, batch.monotone_constraints = handle, trees, kept
    try:
        with pytest.raises(ValueError, match="entry 1"):
            batch.begin(X4, Y4, FOLD, [dict(held_out=0)], monotone_constraints=bad)
        assert batch.handle is handle and batch.trees is trees and batch.monotone_constraints is kept
    finally:
        batch.handle = None


# ---- the restatement does its job on the cases of the GPU tests ---------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_runs():
    """Per case: (the constrained run, the unconstrained trees, the constraint vector), computed once."""
    runs = {}
    for n, nf, depth, lam, mcw, eta in monotone_oracle.CASES:
        x, y = oracle.make_data(n, nf, 5)
        config = dict(max_depth=depth, eta=eta, min_child_weight=mcw, reg_lambda=lam)
        c = monotone_oracle.case_constraints(nf)
        runs[n] = (monotone_oracle.train(x, y, c, monotone_oracle.ROUNDS, **config),
                   oracle.train(x, y, monotone_oracle.ROUNDS, **config), c, (x, y, config))
    return runs


@pytest.mark.parametrize("n", [case[0] for case in monotone_oracle.CASES])
def test_the_constraints_bind_in_every_case(oracle_runs, n):
    constrained, (free_trees, free_margins), c, _ = oracle_runs[n]
    assert constrained["rejected"] > 0
    assert len(constrained["trees"]) == len(free_trees) == monotone_oracle.ROUNDS
    assert not any(monotone_oracle.same_tree(a, b) for a, b in zip(constrained["trees"], free_trees))
    assert constrained["violations"] == [0] * monotone_oracle.ROUNDS
    assert sum(monotone_oracle.violations(tree, c) for tree in free_trees) >= 1
    if n in monotone_oracle.CLAMPING:
        assert constrained["clamped"] >= 1
    assert not np.array_equal(constrained["margins"], free_margins)
    for tree in constrained["trees"]:                 # every node's bounds nest inside its parent's
        for node in np.nonzero(tree["state"] == oracle.SPLIT)[0]:
            for child in (2 * node + 1, 2 * node + 2):
                assert tree["lo"][node] <= tree["lo"][child] <= tree["hi"][child] <= tree["hi"][node]


def test_one_row_gives_the_root_leaf_of_the_unconstrained_rule():
    n, nf, depth, lam, mcw, eta = monotone_oracle.ONE_ROW
    x, y = oracle.make_data(n, nf, 5)
    config = dict(max_depth=depth, eta=eta, min_child_weight=mcw, reg_lambda=lam)
    constrained = monotone_oracle.train(x, y, monotone_oracle.case_constraints(nf), monotone_oracle.ROUNDS, **config)
    free_trees, free_margins = oracle.train(x, y, monotone_oracle.ROUNDS, **config)
    for a, b in zip(constrained["trees"], free_trees):
        assert a["state"][0] == oracle.LEAF and monotone_oracle.same_tree(a, b)
    assert constrained["margins"].tobytes() == free_margins.tobytes()
    assert constrained["rejected"] == 0 and constrained["clamped"] == 0


@pytest.mark.parametrize("n", [case[0] for case in monotone_oracle.CASES])
def test_constraints_that_never_bind_give_the_unconstrained_trees(oracle_runs, n):
    """Constraints on the constant and the all-NaN column alone: no candidate is rejected, no bound gets finite, and
    every number is the unconstrained oracle's, bit for bit."""
    _, (free_trees, free_margins), _, (x, y, config) = oracle_runs[n]
    idle = monotone_oracle.train(x, y, monotone_oracle.idle_constraints(x.shape[1]), monotone_oracle.ROUNDS, **config)
    assert all(monotone_oracle.same_tree(a, b) for a, b in zip(idle["trees"], free_trees))
    assert idle["margins"].tobytes() == free_margins.tobytes()
    assert idle["rejected"] == 0 and idle["clamped"] == 0
    assert all(np.isinf(tree["lo"]).all() and np.isinf(tree["hi"]).all() for tree in idle["trees"])


def test_infinite_bounds_give_the_unconstrained_terms_bit_for_bit():
    rng = np.random.RandomState(3)
    G, H = rng.randn(5000) * 40, rng.rand(5000) * 90
    for lam in (0.0, 0.5, 1.0):
        star, term, clamped = monotone_oracle.bounded(G, H + 1e-3, lam, -np.inf, np.inf)
        assert not clamped.any()
        assert np.array_equal(star, -G / (H + 1e-3 + lam)) and np.array_equal(term, G * G / (H + 1e-3 + lam))
    star, term, clamped = monotone_oracle.bounded(np.array([-2.0, 2.0]), np.array([1.0, 1.0]), 1.0, -0.5, 0.5)
    assert star.tolist() == [0.5, -0.5] and clamped.all()
    assert term.tolist() == [-(2.0 * -2.0 * 0.5 + 2.0 * 0.5 * 0.5), -(2.0 * 2.0 * -0.5 + 2.0 * -0.5 * -0.5)]   # 1.5 each


# ---- ForestModel.monotone_violations ------------------------------------------------------------------------------------
def _arrays(*trees):
    """Flat arrays of trees given as lists of nodes: (feature, threshold, yes, no) for a split, a float for a leaf."""
    feature, threshold, yes, no, offsets = [], [], [], [], [0]
    for nodes in trees:
        for node in nodes:
            split = isinstance(node, tuple)
            feature.append(node[0] if split else -1)
            threshold.append(node[1] if split else node)
            yes.append(node[2] if split else 0)
            no.append(node[3] if split else 0)
        offsets.append(len(feature))
    return dict(feature=np.array(feature, np.int32), threshold=np.array(threshold, np.float32),
                yes=np.array(yes, np.int32), no=np.array(no, np.int32), missing=np.array(yes, np.int32),
                tree_offsets=np.array(offsets, np.int64), base_margin=0.0)


def test_monotone_violations_on_hand_built_trees():
    count = ForestModel.monotone_violations_of
    rising = [(0, 0.5, 1, 2), -1.0, 2.0]                       # x0 < 0.5 -> -1, else 2
    falling = [(0, 0.5, 1, 2), 2.0, -1.0]
    flat = [(0, 0.5, 1, 2), 1.0, 1.0]
    for sign, tree, expected in ((1, rising, 0), (1, falling, 1), (-1, rising, 1), (-1, falling, 0), (0, falling, 0),
                                 (1, flat, 0), (-1, flat, 0)):
        assert count(_arrays(tree), [sign, 0]) == expected, (sign, tree)
    assert count(_arrays(rising, falling, falling, [0.25]), [1, 0]) == 2       # summed over the trees; a lone leaf has none
    assert count(_arrays(falling), [0, 1]) == 0                               # the constraint is on another feature
    # nested: the root splits on x0; its left subtree splits on x1 and holds a leaf (0.9) above the right subtree's
    # smallest (0.5), which breaks x0's +1 although every single split is in order on its own children
    nested = [(0, 0.0, 1, 2), (1, 3.0, 3, 4), (1, 3.0, 5, 6), 0.1, 0.9, 0.5, 1.5]
    assert count(_arrays(nested), [1, 0]) == 1 and count(_arrays(nested), [1, 1]) == 1
    assert count(_arrays(nested), [0, 1]) == 0 and count(_arrays(nested), [0, -1]) == 2
    assert count(_arrays(nested), [-1, 0]) == 1                               # 0.1 < 1.5
    # a child numbered before its parent, as an import may number them (the root is node 0 in every format)
    shuffled = [(0, 0.0, 4, 2), 0.5, (1, 3.0, 1, 3), 1.5, 2.0]
    tree = _arrays(shuffled)
    assert count(tree, [1, 1]) == 1 and count(tree, [-1, 1]) == 0              # x0: left 2.0 > the right side's 0.5
    assert count(tree, [0, -1]) == 1
    assert count(_arrays(), [1, 1]) == 0


def test_monotone_violations_agrees_with_the_oracles_count(oracle_runs):
    """Heap trees of the restatement, turned into model arrays by train.heap_tree, get the oracle's own counts."""
    from doppel_speller_amd.train import heap_tree
    constrained, (free_trees, _), c, (x, _, _) = oracle_runs[300]
    per_feature = oracle.cuts(x)
    offsets = np.concatenate(([0], np.cumsum([cut.size for cut in per_feature]))).astype(np.int32)
    cuts = np.concatenate(per_feature)
    for trees in (constrained["trees"], free_trees):
        parts = [heap_tree(np.stack([t["state"], t["feature"], t["bin"], t["default_left"]], axis=1), t["leaf"], cuts,
                           offsets) for t in trees]
        arrays = ForestModel.extended_arrays(_arrays(), parts)
        assert ForestModel.monotone_violations_of(arrays, c) == sum(monotone_oracle.violations(t, c) for t in trees)


# ---- the C ABI --------------------------------------------------------------------------------------------------------
def test_the_header_declares_both_entries_and_the_binding_lists_them():
    header = open(os.path.join(ROOT, "include", "doppel_amd.h")).read()
    assert re.search(r"\bint ds_trainer_set_monotone\(ds_trainer \*trainer, const int8_t \*constraints\);", header)
    assert re.search(r"\bint ds_trainer_batch_set_monotone\(ds_trainer_batch \*batch, const int8_t \*constraints\);",
                     header)
    assert {"ds_trainer_set_monotone", "ds_trainer_batch_set_monotone"} <= set(_lib.EXPORTED_SYMBOLS)
    assert len(set(_lib.EXPORTED_SYMBOLS)) == len(_lib.EXPORTED_SYMBOLS)
    assert "16 * slots * n_models + n_features" in header            # what ds_trainer_batch_bytes does not count


def test_null_arguments_are_refused_before_any_device_is_touched():
    import doppel_speller_amd as ds
    library = ctypes.CDLL(ds.build_library())
    library.ds_last_error.restype = ctypes.c_char_p
    constraints = np.ones(4, np.int8)
    pointer = constraints.ctypes.data_as(ctypes.c_void_p)
    assert library.ds_trainer_set_monotone(None, pointer) == -1
    assert b"ds_trainer_set_monotone: trainer is null" in library.ds_last_error()
    assert library.ds_trainer_batch_set_monotone(None, pointer) == -1
    assert b"ds_trainer_batch_set_monotone: batch is null" in library.ds_last_error()
