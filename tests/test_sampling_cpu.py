"""Row and column subsampling without a GPU ("Subsampling"): the checks of the four new
parameters at every entry before the library is loaded, the grid rule (no sampling name: the old dicts; one name: four
more keys everywhere), the two new C entries refusing a null handle, the header's declarations, and the invariants of
the NumPy restatement (tests/forest_sampling_oracle.py) that the GPU tests compare against."""
import ctypes
import os
import re

import numpy as np
import pytest

import forest_sampling_oracle as sampling
import forest_train_oracle as oracle
import training_set_oracle
from doppel_speller_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIVE = ["max_depth", "eta", "min_child_weight", "reg_lambda", "beta"]
FOUR = ["subsample", "colsample_bytree", "colsample_bylevel", "sample_seed"]
X, Y = np.zeros((12, 3), np.float32), np.array([0, 1] * 6)

BAD = [
    (dict(subsample=0), "subsample must be a number in"),
    (dict(subsample=1.5), "subsample must be a number in"),
    (dict(subsample=float("nan")), "subsample must be a number in"),
    (dict(subsample="half"), "subsample must be a number in"),
    (dict(colsample_bytree=0.0), "colsample_bytree must be a number in"),
    (dict(colsample_bytree=-0.5), "colsample_bytree must be a number in"),
    (dict(colsample_bylevel=1.0000001), "colsample_bylevel must be a number in"),
    (dict(colsample_bylevel=float("inf")), "colsample_bylevel must be a number in"),
    (dict(sample_seed=-1), "sample_seed must be an integer"),
    (dict(sample_seed=1 << 63), "sample_seed must be an integer"),
    (dict(sample_seed=0.5), "sample_seed must be an integer"),
    (dict(sample_seed=True), "sample_seed must be an integer"),
    (dict(reg_lambda=0, subsample=0.5), "subsample < 1 needs reg_lambda > 0"),
]


@pytest.fixture
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the library was called before the arguments were validated")
    monkeypatch.setattr(_lib, "lib", refuse)


# ---- validation at every entry ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arguments, message", BAD)
def test_every_entry_refuses_before_the_library(no_library, arguments, message):
    import doppel_speller_amd as ds
    from doppel_speller_amd import train, tuning
    device = _lib.DeviceArray.view(4096, (12, 3), np.float32, 0)      # never read: the checks come first
    calls = [
        lambda: train.validate_parameters(**arguments),
        lambda: train.validate_fit(X, Y, **arguments),
        lambda: train.validate_fit_device(device, 12, Y, **arguments),
        lambda: ds.ForestTrainer().begin(X, Y, **arguments),
        lambda: ds.ForestTrainer().fit(X, Y, **arguments),
        lambda: ds.ForestTrainer().begin_device(device, 12, Y, **arguments),
        lambda: ds.ForestTrainer().fit_device(device, 12, Y, **arguments),
        lambda: ds.train_model(["alpha beta", "gamma delta"], [5, 6], ["alpha bet"], [5], top_n=2, sample_n=1,
                               **arguments),
        lambda: ds.parameter_grid(**arguments),
        lambda: tuning.validate_models([dict(arguments, held_out=0)], 3),
        lambda: ds.ForestTrainerBatch().begin(X, Y, np.arange(12) % 3, [dict(arguments, held_out=0)]),
        lambda: ds.ForestTrainerBatch().begin_device(device, 12, Y, np.arange(12) % 3, [dict(arguments)]),
        lambda: ds.cross_validate(X, Y, dict(arguments), n_folds=3),
        lambda: ds.cross_validate(X, Y, [dict(max_depth=2), dict(arguments)], n_folds=3),
        lambda: ds.tune_model_parameters(["alpha beta", "gamma delta"], [5, 6], ["alpha bet", "unknown"], [5, -1],
                                         dict(arguments), n_folds=2, top_n=2, sample_n=1),
    ]
    for call in calls:
        with pytest.raises(ValueError, match=message):
            call()


def test_good_values_pass_and_the_defaults_are_one_and_zero(no_library):
    from doppel_speller_amd import train
    params = train.validate_parameters()
    assert [params[name] for name in FOUR] == [1.0, 1.0, 1.0, 0]
    params = train.validate_parameters(subsample=0.5, colsample_bytree=np.float32(0.25), colsample_bylevel=1,
                                       sample_seed=np.int64((1 << 63) - 1), reg_lambda=1e-9)
    assert [params[name] for name in FOUR] == [0.5, 0.25, 1.0, (1 << 63) - 1]
    assert all(type(params[name]) is float for name in FOUR[:3]) and type(params["sample_seed"]) is int
    assert train.validate_parameters(reg_lambda=0, colsample_bytree=0.5)["reg_lambda"] == 0   # columns alone may
    assert train.validate_fit(X, Y, subsample=0.7)[4]["subsample"] == 0.7
    assert train.SAMPLING_NAMES == tuple(FOUR)


def test_unknown_names_are_still_refused(no_library):
    import doppel_speller_amd as ds
    with pytest.raises(ValueError, match=r"unknown fit parameters \['gamma'\]"):
        ds.train_model(["alpha beta"], [5], ["alpha bet"], [5], gamma=1.0)
    with pytest.raises(ValueError, match=r"unknown fit parameters \['colsample', 'min_split_loss'\]"):
        ds.train_model(["alpha beta"], [5], ["alpha bet"], [5], min_split_loss=1.0, colsample=0.5, subsample=0.5)
    with pytest.raises(ValueError, match=r"unknown parameters \['colsample_bynode'\]"):
        ds.parameter_grid(colsample_bynode=[0.5], subsample=[0.5])
    with pytest.raises(ValueError, match=r"unknown parameters \['gamma'\]"):
        ds.cross_validate(X, Y, dict(gamma=1.0), n_folds=3)
    with pytest.raises(ValueError, match="unknown parameters of model 1"):
        ds.ForestTrainerBatch().begin(X, Y, np.arange(12) % 3, [dict(subsample=0.5), dict(sample=0.5)])
    with pytest.raises(TypeError):
        ds.ForestTrainer().fit(X, Y, gamma=1.0)


# ---- the grid rule ------------------------------------------------------------------------------------------------------
def test_a_grid_without_a_sampling_name_is_the_old_grid(no_library):
    import doppel_speller_amd as ds
    from doppel_speller_amd import tuning
    assert tuning.PARAMETER_NAMES == tuple(FIVE) and tuning.SAMPLING_NAMES == tuple(FOUR)
    assert ds.parameter_grid() == [dict(max_depth=5, eta=0.1, min_child_weight=1.0, reg_lambda=1.0, beta=5.0)]
    grid = ds.parameter_grid(max_depth=[3, 5], beta=[1, 5])
    assert len(grid) == 4 and all(list(one) == FIVE for one in grid)
    sets, _ = tuning.validate_cross_validation([dict(max_depth=2), dict(eta=0.3)], n_folds=3)
    assert all(list(one) == FIVE for one in sets)
    params, held, sets = tuning.validate_models([dict(max_depth=2, held_out=1), dict()], 3)
    assert params.shape == (2, 5) and held.tolist() == [1, -1] and all(list(one) == FIVE for one in sets)


def test_one_sampling_name_puts_all_four_into_every_set(no_library):
    import doppel_speller_amd as ds
    from doppel_speller_amd import tuning
    grid = ds.parameter_grid(max_depth=[3, 5], subsample=[0.5, 1.0])
    assert len(grid) == 4 and all(list(one) == FIVE + FOUR for one in grid)
    assert [(one["max_depth"], one["subsample"]) for one in grid] == [(3, 0.5), (3, 1.0), (5, 0.5), (5, 1.0)]
    assert all(one["colsample_bytree"] == 1.0 and one["colsample_bylevel"] == 1.0 and one["sample_seed"] == 0
               for one in grid)
    # the four vary after beta in their own order, the last-named fastest
    grid = ds.parameter_grid(beta=[1, 5], colsample_bytree=[0.5, 1.0], sample_seed=[0, 7])
    assert [(one["beta"], one["colsample_bytree"], one["sample_seed"]) for one in grid] == \
        [(1, 0.5, 0), (1, 0.5, 7), (1, 1.0, 0), (1, 1.0, 7), (5, 0.5, 0), (5, 0.5, 7), (5, 1.0, 0), (5, 1.0, 7)]
    assert len(ds.parameter_grid(sample_seed=3)) == 1 and list(ds.parameter_grid(sample_seed=3)[0]) == FIVE + FOUR
    # a list of sets of which ONE names one: all carry the four, with defaults
    sets, _ = tuning.validate_cross_validation([dict(max_depth=2), dict(max_depth=2, colsample_bylevel=0.5)], n_folds=3)
    assert all(list(one) == FIVE + FOUR for one in sets)
    assert [one["colsample_bylevel"] for one in sets] == [1.0, 0.5] and sets[0]["subsample"] == 1.0
    params, held, sets = tuning.validate_models([dict(held_out=1), dict(subsample=0.5, sample_seed=9)], 3)
    assert params.shape == (2, 5) and all(list(one) == FIVE + FOUR for one in sets)
    assert [one["sample_seed"] for one in sets] == [0, 9]
    # sets that differ in a sampling parameter alone are different sets; equal ones are still refused
    assert len(tuning.validate_cross_validation([dict(sample_seed=1), dict(sample_seed=2)], n_folds=3)[0]) == 2
    with pytest.raises(ValueError, match="twice"):
        ds.parameter_grid(subsample=[0.5, 0.5])
    with pytest.raises(ValueError, match="twice"):
        tuning.validate_cross_validation([dict(), dict(subsample=1.0)], n_folds=3)
    with pytest.raises(ValueError, match="no values"):
        ds.parameter_grid(subsample=[])


# ---- the C ABI ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def library():
    import doppel_speller_amd as ds
    handle = ctypes.CDLL(ds.build_library())
    handle.ds_last_error.restype = ctypes.c_char_p
    return handle


def test_the_new_entries_refuse_a_null_handle(library):
    d = ctypes.c_double
    assert library.ds_trainer_set_sampling(None, d(0.5), d(0.5), d(0.5), ctypes.c_uint64(1)) == -1
    assert b"ds_trainer_set_sampling: trainer is null" in library.ds_last_error()
    fractions, seeds = np.full(3, 0.5), np.zeros(1, np.uint64)
    pointer = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert library.ds_trainer_batch_set_sampling(None, pointer(fractions), pointer(seeds)) == -1
    assert b"ds_trainer_batch_set_sampling: batch is null" in library.ds_last_error()


def test_the_header_declares_the_entries_and_names_the_purposes():
    with open(os.path.join(ROOT, "include", "doppel_amd.h")) as handle:
        header = handle.read()
    flat = " ".join(header.split())
    assert ("int ds_trainer_set_sampling(ds_trainer *trainer, double subsample, double colsample_bytree, "
            "double colsample_bylevel, uint64_t sample_seed);") in flat
    assert ("int ds_trainer_batch_set_sampling(ds_trainer_batch *batch, const double *fractions, "
            "const uint64_t *sample_seeds);") in flat
    purposes = dict(re.findall(r"#define DS_SAMPLE_PURPOSE_(ROW|TREE|LEVEL) (\d+)", header))
    assert {name: int(value) for name, value in purposes.items()} == \
        dict(ROW=sampling.PURPOSE_ROW, TREE=sampling.PURPOSE_TREE, LEVEL=sampling.PURPOSE_LEVEL)
    used = {training_set_oracle.PURPOSE_MISSPELL, training_set_oracle.PURPOSE_SAMPLE}
    assert len(used | set(int(v) for v in purposes.values())) == 5          # none that ds_training.hip uses
    assert {"ds_trainer_set_sampling", "ds_trainer_batch_set_sampling"} <= set(_lib.EXPORTED_SYMBOLS)


# ---- the oracle's own invariants ----------------------------------------------------------------------------------------
def test_the_stream_is_the_projects_stream():
    rng = np.random.RandomState(5)
    for _ in range(50):
        seed, index = int(rng.randint(0, 1 << 62)) * 2 + 1, (int(rng.randint(0, 1 << 31)) << 32) | int(rng.randint(0, 1 << 31))
        for purpose in (sampling.PURPOSE_ROW, sampling.PURPOSE_TREE, sampling.PURPOSE_LEVEL):
            expected = training_set_oracle.Stream(seed, purpose, index).next()     # the first kept output
            assert sampling.key(seed, purpose, index) == expected
            assert int(sampling.keys(seed, purpose, np.array([index], np.uint64))[0]) == expected


@pytest.mark.parametrize("n_features", [1, 7, 66, 96])
@pytest.mark.parametrize("fraction", [0.01, 0.5, 0.99, 1])
def test_set_sizes_and_the_level_set_is_a_subset_of_the_tree_set(n_features, fraction):
    k_tree = max(1, int(np.floor(fraction * n_features)))
    for tree in range(3):
        of_tree = sampling.tree_set(11, tree, n_features, fraction)
        assert of_tree.size == k_tree == sampling.set_size(fraction, n_features)
        assert np.array_equal(of_tree, np.unique(of_tree)) and of_tree.min() >= 0 and of_tree.max() < n_features
        for level_fraction in (0.01, 0.5, 0.99, 1):
            k_level = max(1, int(np.floor(level_fraction * k_tree)))
            for level in range(3):
                of_level = sampling.level_set(11, tree, level, of_tree, level_fraction)
                assert of_level.size == k_level and set(of_level.tolist()) <= set(of_tree.tolist())
            masks = sampling.level_masks(11, tree, n_features, 3, fraction, level_fraction)
            assert masks.shape == (3, n_features) and (masks.sum(axis=1) == k_level).all()
            assert not masks[:, np.setdiff1d(np.arange(n_features), of_tree)].any()
    if fraction == 1:
        assert np.array_equal(sampling.tree_set(11, 0, n_features, 1), np.arange(n_features))
        assert sampling.level_masks(11, 0, n_features, 2, 1, 1).all()


def test_ties_go_to_the_lower_feature():
    candidates = np.array([2, 5, 7, 9])
    assert sampling._smallest(candidates, np.array([4, 1, 4, 1], np.uint64), 3).tolist() == [2, 5, 9]
    assert sampling._smallest(candidates, np.array([4, 4, 4, 4], np.uint64), 2).tolist() == [2, 5]


def test_the_same_seed_gives_the_same_masks_and_another_seed_others():
    first = sampling.level_masks(3, 2, 66, 5, 0.5, 0.5)
    assert np.array_equal(first, sampling.level_masks(3, 2, 66, 5, 0.5, 0.5))
    assert not np.array_equal(first, sampling.level_masks(4, 2, 66, 5, 0.5, 0.5))
    assert not np.array_equal(first, sampling.level_masks(3, 3, 66, 5, 0.5, 0.5))            # another tree
    assert len({row.tobytes() for row in first}) > 1                                        # the levels differ
    rows = sampling.row_mask(3, 2, 5000, 0.5)
    assert np.array_equal(rows, sampling.row_mask(3, 2, 5000, 0.5))
    assert not np.array_equal(rows, sampling.row_mask(4, 2, 5000, 0.5))
    assert not np.array_equal(rows, sampling.row_mask(3, 1, 5000, 0.5))
    assert 2300 < rows.sum() < 2700                        # 5 sigma of Binomial(5000, 0.5) is 177
    assert sampling.row_mask(3, 2, 5000, 1).all()
    assert 380 < sampling.row_mask(3, 2, 5000, 0.1).sum() < 620


def test_a_rows_draw_depends_on_seed_tree_and_row_alone():
    long = sampling.row_mask(9, 4, 3000, 0.3)
    for n in (1, 63, 64, 65, 1003):
        assert np.array_equal(sampling.row_mask(9, 4, n, 0.3), long[:n])
    for r in (0, 1, 64, 2999):
        x = sampling.key(9, sampling.PURPOSE_ROW, (4 << 32) | r)
        assert bool(long[r]) == ((x >> 11) * 2.0 ** -53 < 0.3)


def test_a_held_out_fold_numbers_the_training_rows_in_row_order():
    """A model that holds a fold out draws for its training rows as a model given those rows alone does."""
    x, y = oracle.make_data(300, 5, 3)
    fold = np.arange(300) % 3
    rng = np.random.RandomState(1)
    rng.shuffle(fold)
    parameters = dict(max_depth=3, eta=0.3, subsample=0.5, colsample_bytree=0.6, sample_seed=5)
    per_feature = oracle.cuts(x)
    whole = sampling.Booster(x, y, parameters, fold, 1, per_feature)
    keep = fold != 1
    subset = sampling.Booster(x[keep], y[keep], parameters, per_feature=per_feature)
    for _ in range(4):
        tree, gh = whole.step()
        subset_tree, subset_gh = subset.step()
        assert not gh[~keep].any() and np.array_equal(gh[keep], subset_gh)
        assert all(np.array_equal(tree[name], subset_tree[name]) for name in tree)
        assert np.array_equal(whole.row_masks[-1][keep], subset.row_masks[-1]) and not whole.row_masks[-1][~keep].any()
    assert np.array_equal(whole.margins()[keep], subset.margins())
    assert sum(int(np.count_nonzero(t["state"] == oracle.SPLIT)) for t in whole.trees) > 8
    assert 0 < whole.row_masks[0].sum() < keep.sum()


def test_defaults_grow_the_existing_oracles_trees():
    x, y = oracle.make_data(400, 6, 8)
    trees, margins, errors = sampling.train(x, y, 3, max_depth=3, eta=0.3)
    expected_trees, expected_margins = oracle.train(x, y, 3, max_depth=3, eta=0.3)
    assert errors == [] and np.array_equal(margins, expected_margins)
    assert all(np.array_equal(a[name], b[name]) for a, b in zip(trees, expected_trees) for name in a)
    sampled, other, _ = sampling.train(x, y, 3, max_depth=3, eta=0.3, subsample=0.5, colsample_bytree=0.5)
    assert not np.array_equal(other, margins)
    for t, tree in enumerate(sampled):                      # every split feature lies in its level's set
        masks = sampling.level_masks(0, t, 6, 3, 0.5, 1.0)
        for node in np.nonzero(tree["state"] == oracle.SPLIT)[0]:
            assert masks[int(np.log2(node + 1)), tree["feature"][node]]
