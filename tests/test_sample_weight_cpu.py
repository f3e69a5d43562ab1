"""Sample weights without a GPU ("Sample weights"): every refusal of validate_sample_weight, the
guard at its edge, the call order of every trainer entry (a bad weight array is refused before the library is reached
and a refused begin keeps the trainer's state), the NumPy restatement's own identities (rows of weight 0 are absent,
all weights 1 is the unweighted rule), kind_weights on a hand-made frame and the C ABI's two new entries."""
import ctypes
import os
import re

import numpy as np
import pytest

import forest_train_oracle as oracle
import forest_weight_oracle as weight_oracle
from doppel_speller_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X4, Y4 = np.zeros((4, 3), np.float32), np.array([0, 1, 0, 1])


@pytest.fixture
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the library was called before the arguments were validated")
    monkeypatch.setattr(_lib, "lib", refuse)


class _Matrix:
    """Stands in for a DeviceArray of a given shape: validation looks at nothing else."""

    def __init__(self, rows, columns):
        self.shape = (rows, columns)


# ---- validate_sample_weight --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights, message", [
    (np.ones((4, 1)), "1-D"),
    (np.float32(1.0), "1-D"),
    (np.ones(3), "4 training rows but 3 sample weights"),
    (np.array(["1", "1", "1", "1"]), "must hold numbers"),
    (np.array([True, True, False, True]), "must hold numbers"),
    (np.array([1, None, 1, 1], object), "must hold numbers"),
    (np.array([1, np.nan, 1, 1]), "NaN or an infinite"),
    (np.array([1, np.inf, 1, 1]), "NaN or an infinite"),
    (np.array([1, 1e39, 1, 1]), "NaN or an infinite"),             # finite as float64, infinite as the float32 it becomes
    (np.array([1, 1, -0.5, 1]), r"negative value \(row 2\)"),
    (np.zeros(4), "total sample weight of the training rows is 0"),
    (np.array([0, 1e-46, 0, 0]), "total sample weight of the training rows is 0"),   # 0 as a float32
    (np.full(4, 2.0 ** 31), "exceeds 2\\^32"),
])
def test_validate_sample_weight_refuses(weights, message):
    import doppel_speller_amd as ds
    with pytest.raises(ValueError, match=message):
        ds.validate_sample_weight(weights, 4)


def test_validate_sample_weight_returns_contiguous_float32():
    import doppel_speller_amd as ds
    for given in ([0, 1, 2, 3], np.arange(8, dtype=np.int64)[::2], np.array([0.1, 1 / 3, 0, 1000]), (1, 1, 1, 1)):
        out = ds.validate_sample_weight(given, 4)
        assert out.dtype == np.float32 and out.shape == (4,) and out.flags["C_CONTIGUOUS"]
        assert np.array_equal(out, np.asarray(given, dtype=np.float32))


def _pieces(total):
    """Three float32 weights whose float64 sum, taken in order, is exactly the float64 `total`."""
    def below(value):                        # the largest float32 <= value: no piece may be negative
        piece = np.float32(value)
        return piece if float(piece) <= value else np.nextafter(piece, np.float32(0.0))
    hi = below(total)
    rest = total - float(hi)
    mid = below(rest)
    lo = np.float32(rest - float(mid))
    weights = np.array([hi, mid, lo], np.float32)
    assert float(weights.astype(np.float64).sum()) == total and (weights >= 0).all()
    return weights


@pytest.mark.parametrize("beta", [5.0, 0.5])
def test_the_guard_at_its_edge(beta):
    """max(beta, 1) * sum(s_r) <= 2^32 with the sum and the product in float64: the last total that passes and the next
    float64 after it, which is the first that does not."""
    import doppel_speller_amd as ds
    factor, limit = max(beta, 1.0), 2.0 ** 32
    last = limit / factor
    while factor * last > limit:
        last = float(np.nextafter(last, 0.0))
    while factor * float(np.nextafter(last, np.inf)) <= limit:
        last = float(np.nextafter(last, np.inf))
    first = float(np.nextafter(last, np.inf))
    assert factor * last <= limit < factor * first
    if beta == 0.5:
        assert last == limit and first == limit + 2.0 ** -20
    else:
        assert abs(last - limit / 5) < 1e-6
    low, high = _pieces(last), _pieces(first)
    assert np.array_equal(ds.validate_sample_weight(low, 3, beta), low)
    with pytest.raises(ValueError, match="exceeds 2\\^32"):
        ds.validate_sample_weight(high, 3, beta)


# ---- call order -----------------------------------------------------------------------------------------------------
BAD = [(np.ones(3), "sample weights"), (np.array([1, -1, 1, 1]), "negative"), (np.array([1, np.nan, 1, 1]), "NaN"),
       (np.zeros(4), "is 0"), (np.ones((4, 1)), "1-D")]


@pytest.mark.parametrize("weights, message", BAD)
def test_a_bad_sample_weight_is_refused_before_the_library(no_library, weights, message):
    import doppel_speller_amd as ds
    fold = np.array([0, 1, 0, 1])
    calls = [lambda: ds.ForestTrainer().begin(X4, Y4, sample_weight=weights),
             lambda: ds.ForestTrainer().fit(X4, Y4, sample_weight=weights, num_boost_round=2),
             lambda: ds.ForestTrainer().begin_device(_Matrix(4, 3), 4, Y4, sample_weight=weights),
             lambda: ds.ForestTrainer().fit_device(_Matrix(4, 3), 4, Y4, sample_weight=weights),
             lambda: ds.ForestTrainerBatch().begin(X4, Y4, fold, [dict(held_out=0)], sample_weight=weights),
             lambda: ds.ForestTrainerBatch().begin_device(_Matrix(4, 3), 4, Y4, fold, [dict(held_out=0)],
                                                          sample_weight=weights)]
    for call in calls:
        with pytest.raises(ValueError, match=message):
            call()


def test_the_guard_takes_the_trainers_beta_and_the_batchs_largest(no_library):
    import doppel_speller_amd as ds
    weights = np.full(4, 2.0 ** 28, np.float32)              # total 2^30: fine up to beta 4
    fold = np.array([0, 1, 0, 1])
    with pytest.raises(AssertionError, match="before the arguments were validated"):
        ds.ForestTrainer().begin(X4, Y4, sample_weight=weights, beta=4.0)
    with pytest.raises(ValueError, match="exceeds 2\\^32"):
        ds.ForestTrainer().begin(X4, Y4, sample_weight=weights)                    # the default beta, 5
    with pytest.raises(AssertionError, match="before the arguments were validated"):
        ds.ForestTrainerBatch().begin(X4, Y4, fold, [dict(beta=4.0), dict(beta=1.0)], sample_weight=weights)
    with pytest.raises(ValueError, match="exceeds 2\\^32"):
        ds.ForestTrainerBatch().begin(X4, Y4, fold, [dict(beta=1.0), dict(beta=4.5)], sample_weight=weights)


def test_a_batch_model_whose_training_rows_weigh_nothing_is_named(no_library):
    import doppel_speller_amd as ds
    fold = np.array([0, 1, 0, 1])
    weights = np.array([0, 2, 0, 0.5])                       # fold 0 weighs nothing: the model that holds fold 1 out
    models = [dict(held_out=0), dict(held_out=-1), dict(held_out=1), dict(held_out=1)]
    for begin in (lambda: ds.ForestTrainerBatch().begin(X4, Y4, fold, models, sample_weight=weights),
                  lambda: ds.ForestTrainerBatch().begin_device(_Matrix(4, 3), 4, Y4, fold, models,
                                                               sample_weight=weights)):
        with pytest.raises(ValueError, match=r"model 2: the total sample weight of its training rows \(outside fold 1\)"):
            begin()
    with pytest.raises(AssertionError, match="before the arguments were validated"):
        ds.ForestTrainerBatch().begin(X4, Y4, fold, models[:2], sample_weight=weights)
    with pytest.raises(ValueError, match="model 1: the total sample weight"):
        ds.cross_validate(X4, Y4, dict(max_depth=2), n_folds=2, groups=fold, sample_weight=weights)


def test_a_refused_second_begin_keeps_the_first_state(no_library):
    import doppel_speller_amd as ds
    trainer = ds.ForestTrainer()
    handle, trees, params, kept = ctypes.c_void_p(1), [object()], dict(max_depth=2), np.ones(4, np.float32)
    trainer.handle, trainer.trees, trainer.params, trainer.sample_weight = handle, trees, params, kept
    bad = np.array([1, -1, 1, 1])
    try:
        for again in (lambda: trainer.begin(X4, Y4, sample_weight=bad), lambda: trainer.fit(X4, Y4, sample_weight=bad),
                      lambda: trainer.begin_device(_Matrix(4, 3), 4, Y4, sample_weight=bad),
                      lambda: trainer.fit_device(_Matrix(4, 3), 4, Y4, sample_weight=bad)):
            with pytest.raises(ValueError, match="negative"):
                again()
            assert trainer.handle is handle and trainer.trees is trees and trainer.params is params
            assert trainer.sample_weight is kept
    finally:
        trainer.handle = None                      # the stand-in is nothing the library could give back
    batch = ds.ForestTrainerBatch()
    batch.handle, batch.trees, batch.sample_weight = handle, trees, kept
    try:
        with pytest.raises(ValueError, match="negative"):
            batch.begin(X4, Y4, np.array([0, 1, 0, 1]), [dict(held_out=0)], sample_weight=bad)
        assert batch.handle is handle and batch.trees is trees and batch.sample_weight is kept
    finally:
        batch.handle = None


def test_fit_with_sample_weight_reaches_the_library(no_library):
    """The argument is known to all four forms and both batch forms, by keyword: with a legal array each gets past its
    checks to the library (the fixture's refusal)."""
    import doppel_speller_amd as ds
    w = np.array([0.5, 1, 0, 2])
    fold = np.array([0, 1, 0, 1])
    for call in (lambda: ds.ForestTrainer().fit(X4, Y4, sample_weight=w),
                 lambda: ds.ForestTrainer().begin(X4, Y4, sample_weight=w),
                 lambda: ds.ForestTrainer().fit_device(_Matrix(4, 3), 4, Y4, sample_weight=w),
                 lambda: ds.ForestTrainer().begin_device(_Matrix(4, 3), 4, Y4, sample_weight=w),
                 lambda: ds.ForestTrainerBatch().begin(X4, Y4, fold, [dict(held_out=0)], sample_weight=w),
                 lambda: ds.ForestTrainerBatch().begin_device(_Matrix(4, 3), 4, Y4, fold, [dict(held_out=0)],
                                                              sample_weight=w),
                 lambda: ds.cross_validate(X4, Y4, dict(max_depth=2), n_folds=2, sample_weight=w)):
        with pytest.raises(AssertionError, match="before the arguments were validated"):
            call()
    assert ds.ForestTrainer().sample_weight is None and ds.ForestTrainerBatch().sample_weight is None
    with pytest.raises(TypeError):
        ds.ForestTrainer().fit(X4, Y4, None, None, w)          # by keyword only


def test_train_model_and_tuning_validate_kind_weights_before_the_library(no_library):
    import doppel_speller_amd as ds
    good = dict(truth_titles=["alpha beta", "gamma delta", "epsilon zeta"], truth_title_ids=[5, 6, 7],
                train_titles=["alpha bet", "unknown"], train_title_ids=[5, -1], top_n=2, sample_n=1)
    for weights, message in ((dict(neutral=2), "unknown kind weights"), (dict(positive=-1), "positive rows"),
                             (dict(generated=float("nan")), "generated rows"), ([1, 2, 3], "must be a dict")):
        with pytest.raises(ValueError, match=message):
            ds.train_model(**good, kind_weights=weights)
        with pytest.raises(ValueError, match=message):
            ds.tune_model_parameters(**good, parameters=dict(max_depth=2), n_folds=2, kind_weights=weights)


# ---- the restatement's own identities --------------------------------------------------------------------------------
@pytest.mark.parametrize("n, nf, depth", [(1, 3, 1), (9, 6, 3), (300, 10, 4), (1000, 12, 5)])
def test_rows_of_weight_zero_are_absent_in_the_oracle(n, nf, depth):
    """A matrix stacked on a copy of itself with flipped labels and weight 0, all rows permuted, grows the trees, leaf
    bits and margins of the matrix alone; its cuts are the matrix's, and every sum is an integer below 2^62."""
    x, y = oracle.make_data(n, nf, 50 + n)
    weights = weight_oracle.draw_weights(n, 60 + n)
    x2, y2, w2, where = weight_oracle.stacked(x, y, weights, 70 + n)
    config = dict(max_depth=depth, eta=0.3, min_child_weight=0.5, reg_lambda=1.0)
    trees, margins, cuts, every_gh = weight_oracle.train(x, y, weights, 4, **config)
    trees2, margins2, cuts2, every_gh2 = weight_oracle.train(x2, y2, w2, 4, **config)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(cuts, cuts2))
    for a, b in zip(trees, trees2):
        assert weight_oracle.same_tree(a, b)
    assert np.array_equal(margins.view(np.uint32), margins2[where].view(np.uint32))
    for gh, gh2 in zip(every_gh, every_gh2):
        assert gh.dtype == np.int64 and np.array_equal(gh, gh2[where])
        assert not gh2[w2 == 0].any()
        totals = [sum(int(v) for v in gh2[:, k]) for k in range(2)]            # Python integers: no overflow possible
        assert totals == [sum(int(v) for v in gh[:, k]) for k in range(2)]
        assert all(abs(total) < 2 ** 62 for total in totals)
    if n >= 300:
        assert any(np.count_nonzero(tree["state"] == oracle.SPLIT) >= 3 for tree in trees)


def test_all_ones_is_the_unweighted_oracle():
    rng = np.random.RandomState(5)
    p = rng.rand(4000).astype(np.float32)
    p[:4] = (0.0, 1.0, np.float32(1e-30), np.nextafter(np.float32(1.0), np.float32(0.0)))
    y = (rng.rand(4000) < 0.3).astype(np.float32)
    for beta in (5.0, 0.5, 1.0):
        assert np.array_equal(weight_oracle.gradients(p, y, np.ones(4000, np.float32), beta), oracle.gradients(p, y, beta))
    weights = weight_oracle.draw_weights(4000, 6)
    weighted = weight_oracle.gradients(p, y, weights, 5.0)
    assert not weighted[weights == 0].any()
    doubled = weights == 2
    # 2 g is exact, so only the two roundings differ: |rint(2 q) - 2 rint(q)| <= 1
    assert np.abs(weighted[doubled] - 2 * oracle.gradients(p, y, 5.0)[doubled]).max() <= 1
    assert set(np.unique(weights)) == set(weight_oracle.WEIGHT_VALUES.astype(np.float32))


# ---- kind_weights ----------------------------------------------------------------------------------------------------
def test_kind_weights_on_a_hand_made_frame():
    import pandas as pd

    import doppel_speller_amd as ds
    from doppel_speller_amd import training_set
    rows = pd.DataFrame({"kind": np.array([2, 2, 3, 3, 3, 1, 1, 2], np.uint8),
                         "query_index": np.arange(8), "truth_row": np.arange(8), "target": np.zeros(8, np.float32),
                         "evaluation": np.array([0, 1, 0, 0, 1, 0, 0, 0], bool)})
    out = ds.kind_weights(rows, dict(generated=0.5, negative=0.25, positive=2))
    assert out.dtype == np.float32 and out.flags["C_CONTIGUOUS"]
    assert out.tolist() == [0.25, 2.0, 2.0, 0.5, 0.5, 0.25]              # frame order, evaluation rows 1 and 4 dropped
    assert ds.kind_weights(rows, dict(positive=3)).tolist() == [1.0, 3.0, 3.0, 1.0, 1.0, 1.0]     # a missing name: 1.0
    assert ds.kind_weights(rows, {}).tolist() == [1.0] * 6
    assert ds.kind_weights(rows, dict(negative=0)).tolist() == [0.0, 1.0, 1.0, 1.0, 1.0, 0.0]
    with pytest.raises(ValueError, match=r"unknown kind weights \['neutral'\]"):
        ds.kind_weights(rows, dict(neutral=2.0))
    with pytest.raises(ValueError, match="negative rows"):
        ds.kind_weights(rows, dict(negative=-1.0))
    with pytest.raises(ValueError, match="must be a dict"):
        ds.kind_weights(rows, None)
    assert ds.kind_weights is training_set.kind_weights
    assert ds.kind_weights(rows.iloc[:0], dict(positive=3)).shape == (0,)


# ---- the C ABI --------------------------------------------------------------------------------------------------------
def test_the_header_declares_both_entries_and_the_binding_lists_them():
    header = open(os.path.join(ROOT, "include", "doppel_amd.h")).read()
    assert re.search(r"\bint ds_trainer_set_weights\(ds_trainer \*trainer, const float \*weights\);", header)
    assert re.search(r"\bint ds_trainer_batch_set_weights\(ds_trainer_batch \*batch, const float \*weights\);", header)
    assert {"ds_trainer_set_weights", "ds_trainer_batch_set_weights"} <= set(_lib.EXPORTED_SYMBOLS)
    assert len(set(_lib.EXPORTED_SYMBOLS)) == len(_lib.EXPORTED_SYMBOLS)


def test_null_arguments_are_refused_before_any_device_is_touched():
    import doppel_speller_amd as ds
    library = ctypes.CDLL(ds.build_library())
    library.ds_last_error.restype = ctypes.c_char_p
    weights = np.ones(4, np.float32)
    pointer = weights.ctypes.data_as(ctypes.c_void_p)
    assert library.ds_trainer_set_weights(None, pointer) == -1
    assert b"ds_trainer_set_weights: trainer is null" in library.ds_last_error()
    assert library.ds_trainer_batch_set_weights(None, pointer) == -1
    assert b"ds_trainer_batch_set_weights: batch is null" in library.ds_last_error()
