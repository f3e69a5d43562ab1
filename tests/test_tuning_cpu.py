"""Cross-validation and tuning without a GPU: the fold assignment, the parameter grid, xgb.cv's choice on hand-written
integer curves, the oracle's own consistency (held-out rows with zero gradients = training on the subset), the
argument checks of cross_validate / tune_model_parameters before the library is loaded, and the argument errors of
the ds_trainer_batch_* entry points, which refuse before they touch a device."""
import ctypes

import numpy as np
import pytest

import forest_cv_oracle as cv_oracle
import forest_train_oracle as oracle
from doppel_speller_amd import _lib


@pytest.fixture
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the library was called before the arguments were validated")
    monkeypatch.setattr(_lib, "lib", refuse)


# ---- fold_assignment ---------------------------------------------------------------------------------------------------
def test_fold_assignment_keeps_groups_whole_and_balanced():
    import doppel_speller_amd as ds
    rng = np.random.RandomState(1)
    groups = rng.randint(0, 103, 2000) * 7 - 50              # 103 groups of unequal size, not 0..G-1
    folds = ds.fold_assignment(groups, 5, seed=3)
    assert folds.dtype == np.uint8 and folds.shape == (2000,) and set(folds.tolist()) == set(range(5))
    distinct = np.unique(groups)
    fold_of = {}
    for g, f in zip(groups.tolist(), folds.tolist()):
        assert fold_of.setdefault(g, f) == f                  # rows of one group share a fold
    per_fold = np.bincount([fold_of[g] for g in distinct.tolist()], minlength=5)
    assert per_fold.sum() == distinct.shape[0] and per_fold.max() - per_fold.min() <= 1
    # the documented rule, restated
    order = distinct[np.random.default_rng(3).permutation(distinct.shape[0])]
    assert all(fold_of[g] == i % 5 for i, g in enumerate(order.tolist()))


def test_fold_assignment_depends_on_seed_and_not_on_row_order():
    import doppel_speller_amd as ds
    rng = np.random.RandomState(2)
    groups = rng.randint(0, 60, 700)
    first = ds.fold_assignment(groups, 4, seed=11)
    assert np.array_equal(first, ds.fold_assignment(groups.copy(), 4, seed=11))
    assert not np.array_equal(first, ds.fold_assignment(groups, 4, seed=12))
    order = rng.permutation(700)
    assert np.array_equal(ds.fold_assignment(groups[order], 4, seed=11), first[order])
    own = ds.fold_assignment(None, 3, seed=0, n=10)           # every row its own group
    assert np.bincount(own, minlength=3).tolist() in ([4, 3, 3],) and own.dtype == np.uint8
    assert np.array_equal(own, ds.fold_assignment(np.arange(10), 3, seed=0))


@pytest.mark.parametrize("arguments, message", [
    (dict(n_folds=1), "n_folds"),
    (dict(n_folds=256), "n_folds"),
    (dict(n_folds=True), "n_folds"),
    (dict(n_folds=7), "exceeds the 6 groups"),
    (dict(groups=np.zeros((3, 2))), "1-D"),
    (dict(seed=-1), "seed"),
    (dict(groups=None), "without groups the number of rows is needed"),
    (dict(groups=None, n=0), "n must be"),
    (dict(n=7), "7 rows but 8 groups"),
])
def test_fold_assignment_errors(arguments, message):
    import doppel_speller_amd as ds
    call = dict(dict(groups=np.array([0, 1, 2, 3, 4, 5, 5, 5]), n_folds=3, seed=0), **arguments)
    with pytest.raises(ValueError, match=message):
        ds.fold_assignment(**call)


# ---- parameter_grid ----------------------------------------------------------------------------------------------------
def test_parameter_grid_order_and_broadcasting():
    import doppel_speller_amd as ds
    grid = ds.parameter_grid(max_depth=[3, 5], eta=0.3, beta=[1, 5, 9])
    assert len(grid) == 6
    assert [(g["max_depth"], g["beta"]) for g in grid] == [(3, 1), (3, 5), (3, 9), (5, 1), (5, 5), (5, 9)]   # last fastest
    assert all(g["eta"] == 0.3 and g["min_child_weight"] == 1.0 and g["reg_lambda"] == 1.0 for g in grid)
    assert all(list(g) == ["max_depth", "eta", "min_child_weight", "reg_lambda", "beta"] for g in grid)
    assert ds.parameter_grid() == [dict(max_depth=5, eta=0.1, min_child_weight=1.0, reg_lambda=1.0, beta=5.0)]
    both = ds.parameter_grid(eta=[0.1, 0.2], reg_lambda=[0.0, 1.0])
    assert [(g["eta"], g["reg_lambda"]) for g in both] == [(0.1, 0.0), (0.1, 1.0), (0.2, 0.0), (0.2, 1.0)]


@pytest.mark.parametrize("lists, message", [
    (dict(max_depth=[3, 3]), "twice"),
    (dict(eta=[0.1, 0.10]), "twice"),
    (dict(max_depth=[3, 9]), "max_depth"),
    (dict(eta=[0.1, 0]), "eta"),
    (dict(reg_lambda=0, min_child_weight=[1, 0]), "cannot both be 0"),
    (dict(beta=[]), "no values"),
    (dict(depth=[3]), "unknown parameters"),
])
def test_parameter_grid_refuses(lists, message):
    import doppel_speller_amd as ds
    with pytest.raises(ValueError, match=message):
        ds.parameter_grid(**lists)


# ---- select_parameters -------------------------------------------------------------------------------------------------
def test_select_parameters_first_minimum_and_ties():
    import doppel_speller_amd as ds
    # set 0: summed 9 5 5 7 -> first minimum at round 1; set 1: summed 9 8 5 5 -> round 2, the same error
    histories = [[[5, 3, 2, 4], [4, 2, 3, 3]], [[5, 4, 3, 2], [4, 4, 2, 3]]]
    chosen = ds.select_parameters(histories)
    assert chosen["history"] == [[9, 5, 5, 7], [9, 8, 5, 5]]
    assert chosen["best_iteration"] == [1, 2] and chosen["error"] == [5, 5] and chosen["rounds"] == [4, 4]
    assert chosen["chosen"] == 0                               # tie on the error: the smaller best_iteration
    assert ds.select_parameters(histories[::-1])["chosen"] == 1
    # tie on error and best_iteration: the earlier set
    same = [[[3, 1, 2]], [[4, 1, 1]], [[2, 2, 2]]]
    assert ds.select_parameters(same)["chosen"] == 0 and ds.select_parameters(same)["best_iteration"] == [1, 1, 0]
    assert ds.select_parameters([[[7, 6]], [[9, 2]]])["chosen"] == 1          # the lowest error wins over the order


def test_select_parameters_with_a_set_that_stopped_earlier():
    import doppel_speller_amd as ds
    early = [[4, 3, 5, 5, 5], [4, 3, 4, 4, 4]]                # summed 8 6 9 9 9: stopped 3 rounds after round 1
    late = [[4, 4, 4, 3, 3, 2, 1, 3], [4, 4, 4, 4, 3, 3, 2, 3]]   # summed 8 8 8 7 6 5 3 6
    chosen = ds.select_parameters([early, late], early_stopping_rounds=3)
    assert chosen["rounds"] == [5, 8] and chosen["best_iteration"] == [1, 6] and chosen["error"] == [6, 3]
    assert chosen["chosen"] == 1
    # entries past a set's stopping round are not looked at: 0 at round 6 would otherwise win
    longer = [[[8, 6, 9, 9, 9, 9, 0]], [[7, 7, 7]]]
    chosen = ds.select_parameters(longer, early_stopping_rounds=3)
    assert chosen["rounds"] == [5, 3] and chosen["error"] == [6, 7] and chosen["history"][0] == [8, 6, 9, 9, 9]
    assert ds.select_parameters(longer)["error"] == [0, 7]
    with pytest.raises(ValueError, match="one length"):
        ds.select_parameters([[[1, 2], [1]]])
    with pytest.raises(ValueError, match="early_stopping_rounds"):
        ds.select_parameters([[[1, 2]]], early_stopping_rounds=0)


# curve, then {early_stopping_rounds: (best_iteration, rounds)} worked out by hand; None never stops
CURVES = {
    "falling": ([9, 7, 5, 3, 1], {1: (4, 5), 3: (4, 5), None: (4, 5)}),
    "minimum_first": ([2, 5, 6, 7, 8, 9], {1: (0, 2), 3: (0, 4), None: (0, 6)}),
    "equal_minima": ([5, 3, 4, 3, 6, 7, 8], {1: (1, 3), 3: (1, 5), None: (1, 7)}),            # the first wins
    "minimum_one_before_the_end": ([9, 8, 2, 5], {1: (2, 4), 3: (2, 4), None: (2, 4)}),
    "minimum_three_before_the_end": ([9, 8, 2, 5, 5, 5], {1: (2, 4), 3: (2, 6), None: (2, 6)}),
    "one_round": ([4], {1: (0, 1), 3: (0, 1), None: (0, 1)}),
}


@pytest.mark.parametrize("patience", [1, 3, None])
@pytest.mark.parametrize("name", sorted(CURVES))
def test_fit_stops_where_select_parameters_stops(name, patience):
    """ForestTrainer._boost, stepped through a hand-made curve, keeps the round and grows the rounds that
    select_parameters reports for that curve."""
    import doppel_speller_amd as ds
    curve, expected = CURVES[name]
    trainer = ds.ForestTrainer()
    errors = iter(curve)

    def step():
        trainer.trees.append(None)
        trainer.history.append(next(errors))
        return trainer.history[-1]
    trainer.step, trainer.model = step, lambda n_trees: n_trees
    kept = trainer._boost(dict(num_boost_round=len(curve),
                               early_stopping_rounds=len(curve) + 1 if patience is None else patience))
    chosen = ds.select_parameters([[curve]], patience)
    assert (trainer.best_iteration, len(trainer.trees)) == expected[patience]
    assert (chosen["best_iteration"][0], chosen["rounds"][0]) == expected[patience]
    assert kept == trainer.best_iteration + 1 and trainer.history == chosen["history"][0]
    assert chosen["error"][0] == curve[trainer.best_iteration]


# ---- the oracle's own consistency --------------------------------------------------------------------------------------
def test_zeroed_gradients_train_the_subset_trees():
    """300 rows x 4 features, 3 folds, depth 3, 5 rounds: growing on all rows with the held-out rows' (g, h) zeroed gives
    the trees of growing on the training rows' columns of the same bins, and so the same margins."""
    import doppel_speller_amd as ds
    x, y = oracle.make_data(300, 4, 17)
    fold = ds.fold_assignment(None, 3, seed=1, n=300)
    per_feature = oracle.cuts(x)
    node_bins = oracle.bins(x, per_feature)
    counts = np.array([c.size for c in per_feature])
    splits = 0
    for held_out in range(3):
        model = dict(cv_oracle.DEFAULTS, max_depth=3, eta=0.3, held_out=held_out)
        leafsum = np.zeros(300, np.float32)
        for _ in range(5):
            gh = oracle.gradients(oracle.sigmoid32(np.float32(0.0) + leafsum), y, 5.0)
            tree, leaves = cv_oracle.grow(node_bins, counts, gh, fold, model)
            subset_tree, subset_leaves = cv_oracle.grow_on_subset(node_bins, counts, gh, fold, model)
            assert cv_oracle.same_tree(tree, subset_tree)
            keep = fold != held_out
            assert np.array_equal(leaves[keep].view(np.uint32), subset_leaves.view(np.uint32))
            leafsum = (leafsum + leaves).astype(np.float32)
            splits += int(np.count_nonzero(tree["state"] == oracle.SPLIT))
    assert splits > 30
    trees, margins, errors = cv_oracle.train(x, y, fold, dict(cv_oracle.DEFAULTS, max_depth=3, eta=0.3, held_out=2), 5)
    assert cv_oracle.same_tree(trees[-1], tree) and np.array_equal(margins, np.float32(0.0) + leafsum)
    assert len(errors) == 5 and all(isinstance(e, int) for e in errors)


# ---- argument errors before the library --------------------------------------------------------------------------------
X, Y = np.zeros((12, 3), np.float32), np.array([0, 1] * 6)


@pytest.mark.parametrize("arguments, message", [
    (dict(parameters=[]), "non-empty"),
    (dict(parameters=dict(depth=3)), "unknown parameters"),
    (dict(parameters=dict(max_depth=9)), "max_depth"),
    (dict(parameters=[dict(eta=0.1), dict(eta=0.1)]), "twice"),
    (dict(parameters=[dict(reg_lambda=0, min_child_weight=0)]), "cannot both be 0"),
    (dict(n_folds=1), "n_folds"),
    (dict(n_folds=13), "exceeds the 12 groups"),
    (dict(groups=np.zeros(12)), "exceeds the 1 groups"),
    (dict(groups=np.arange(11)), "12 rows but 11 groups"),
    (dict(seed=-1), "seed"),
    (dict(num_boost_round=0), "num_boost_round"),
    (dict(early_stopping_rounds=0), "early_stopping_rounds"),
    (dict(max_bin=1), "max_bin"),
    (dict(models_per_batch=2), "below n_folds"),
    (dict(models_per_batch=257), "models_per_batch"),
    (dict(features=np.zeros((12, 97), np.float32)), "97 columns"),
    (dict(target=np.arange(12)), "labels must all be 0 or 1"),
    (dict(target=np.zeros(11)), "12 training rows but 11 labels"),
])
def test_cross_validate_validates_before_the_library(no_library, arguments, message):
    import doppel_speller_amd as ds
    call = dict(dict(features=X, target=Y, parameters=dict(max_depth=2), n_folds=3), **arguments)
    with pytest.raises(ValueError, match=message):
        ds.cross_validate(**call)


GOOD = dict(truth_titles=["alpha beta", "gamma delta", "epsilon zeta"], truth_title_ids=[5, 6, 7],
            train_titles=["alpha bet", "unknown"], train_title_ids=[5, -1], top_n=2, sample_n=1,
            parameters=dict(max_depth=2), n_folds=2)


@pytest.mark.parametrize("change, message", [
    (dict(train_title_ids=[5]), "train title ids"),
    (dict(sample_n=3), "exceeds top_n"),
    (dict(seed=-1), "seed"),
    (dict(parameters=dict(max_depth=0)), "max_depth"),
    (dict(parameters=[dict(), dict()]), "twice"),
    (dict(n_folds=0), "n_folds"),
    (dict(num_boost_round=0), "num_boost_round"),
    (dict(early_stopping_rounds=True), "early_stopping_rounds"),
    (dict(models_per_batch=1), "below n_folds"),
    (dict(refit=False), "unknown cross-validation arguments"),
    (dict(evaluation_fractions={}), "unknown cross-validation arguments"),
])
def test_tune_model_parameters_validates_before_the_library(no_library, change, message):
    import doppel_speller_amd as ds
    with pytest.raises(ValueError, match=message):
        ds.tune_model_parameters(**dict(GOOD, **change))


def test_trainer_batch_validates_before_the_library(no_library):
    import doppel_speller_amd as ds
    fold = np.arange(12) % 3
    good = [dict(max_depth=2, held_out=0)]
    for arguments, message in (
            (dict(models=[]), "1 to 256 models"), (dict(models=[dict()] * 257), "1 to 256 models"),
            (dict(models=[dict(max_depth=9)]), "max_depth"), (dict(models=[dict(held_out=3)]), "held_out = 3"),
            (dict(models=[dict(held_out=-2)]), "held_out"), (dict(models=[dict(depth=1)]), "unknown parameters of model 0"),
            (dict(fold=np.arange(11)), "12 rows but 11 fold entries"), (dict(fold=np.full(12, 255)), "fold must hold"),
            (dict(fold=np.zeros(12)), "fold must hold"), (dict(max_bin=1), "max_bin")):
        with pytest.raises(ValueError, match=message):
            ds.ForestTrainerBatch().begin(**dict(dict(features=X, target=Y, fold=fold, models=good), **arguments))
    with pytest.raises(RuntimeError, match="before begin"):
        ds.ForestTrainerBatch().step()


# ---- the C ABI refuses before it touches a device ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def library():
    import doppel_speller_amd as ds
    handle = ctypes.CDLL(ds.build_library())
    handle.ds_last_error.restype = ctypes.c_char_p
    handle.ds_trainer_batch_bytes.restype = ctypes.c_int64
    handle.ds_trainer_batch_bytes.argtypes = [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]
    return handle


from trainer_batch_cases import _p, batch_create_cases, call_batch_create  # noqa: E402


@pytest.mark.parametrize("entry", ["ds_trainer_batch_create", "ds_trainer_batch_create_device"])
def test_batch_create_argument_errors(library, entry):
    for changes, message in batch_create_cases():
        status, handle, error = call_batch_create(library, entry, **changes)
        assert status == -1 and not handle and message in error and error.startswith(entry + ":"), (changes, error)
    arrays = np.zeros(8, np.float64)
    assert getattr(library, entry)(_p(arrays), ctypes.c_int64(4), 2, _p(arrays), _p(arrays), _p(arrays), _p(arrays), 3, 2,
                                   _p(arrays), _p(arrays), 0, None) == -1
    assert b"out is null" in library.ds_last_error()


def test_batch_entry_points_refuse_null_and_unknown(library):
    buffer = np.zeros(64, np.int64)
    assert library.ds_trainer_batch_step(None, None, _p(buffer), _p(buffer), _p(buffer)) == -1
    assert b"ds_trainer_batch_step: null argument" in library.ds_last_error()
    assert library.ds_trainer_batch_read(None, 0, None, None, None, None) == -1
    assert b"batch is null" in library.ds_last_error()
    library.ds_trainer_batch_destroy(None)
    assert library.ds_trainer_batch_option(None, ctypes.c_int64(1)) == -1
    assert b"ds_trainer_batch_option: null name" in library.ds_last_error()
    assert library.ds_trainer_batch_option(b"blocks", ctypes.c_int64(1)) == -1
    assert b"unknown option" in library.ds_last_error()
    assert library.ds_trainer_batch_option(b"max_blocks", ctypes.c_int64(-1)) == -1
    assert b"max_blocks" in library.ds_last_error()


def test_batch_bytes_formula(library):
    bytes_ = library.ds_trainer_batch_bytes
    for arguments in ((0, 4, 1, 5), (2 ** 31, 4, 1, 5), (10, 0, 1, 5), (10, 97, 1, 5), (10, 4, 0, 5), (10, 4, 257, 5),
                      (10, 4, 1, 0), (10, 4, 1, 9)):
        assert bytes_(*arguments) == -1
    n, nf = 1000, 7
    one, two = bytes_(n, nf, 1, 5), bytes_(n, nf, 2, 5)
    shared = n * nf + 5 * n
    per_model = two - one
    assert one - per_model == shared                                       # bins, labels, folds
    assert 28 * n + 31 * nf * 4096 <= per_model <= 28 * n + 31 * nf * 4096 + 16384   # rows, histograms, a few KiB
    assert bytes_(n, nf, 256, 8) - bytes_(n, nf, 255, 8) >= 28 * n + 255 * nf * 4096
    assert bytes_(2 ** 31 - 1, 96, 256, 8) > 2 ** 43                       # no overflow at the limits
