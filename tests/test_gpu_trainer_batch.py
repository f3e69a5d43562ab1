"""ForestTrainerBatch on the GPU (csrc/ds_train_batch.hip): against ForestTrainer on each fold's training rows, against
the NumPy restatement (tests/forest_cv_oracle.py) with mixed parameters, with inactive models, at the limits of the
C ABI, and the ABI's refusals.  Everything is compared bit for bit."""
import ctypes

import numpy as np
import pytest

import forest_cv_oracle as cv_oracle
import forest_train_oracle as oracle
from forest_train_oracle import make_data
from trainer_batch_cases import _p

pytestmark = pytest.mark.gpu


def heap_equal(device, expected):
    """A batch heap (slots of the batch's largest depth) against an oracle heap (slots of the model's own depth)."""
    info, leaf = device
    slots = expected["state"].shape[0]
    assert not info[slots:, 0].any()                      # nothing beyond the model's own depth
    info, leaf = info[:slots], leaf[:slots]
    assert np.array_equal(info[:, 0], expected["state"])
    split = expected["state"] == oracle.SPLIT
    assert np.array_equal(info[split, 1], expected["feature"][split])
    assert np.array_equal(info[split, 2], expected["bin"][split])
    assert np.array_equal(info[split, 3], expected["default_left"][split])
    leaves = expected["state"] == oracle.LEAF
    assert np.array_equal(leaf[leaves].view(np.uint32), expected["leaf"][leaves].view(np.uint32))


# ---- 1. against the parent's own trainer ------------------------------------------------------------------------------
def test_every_fold_equals_forest_trainer_on_its_training_rows():
    """6,000 rows x 5 integer-valued features, 3 folds, depth 3: every feature has the same distinct values in each
    fold's training part as in the whole matrix, so ForestTrainer's own cuts of the subset are the batch's cuts, and
    its trees, training margins and evaluation errors must be the batch's."""
    import doppel_speller_amd as ds
    rng = np.random.RandomState(31)
    x = rng.randint(0, 20, (6000, 5)).astype(np.float32)
    y = (x[:, 0] + x[:, 1] - 0.5 * x[:, 2] + rng.randn(6000) * 3 > 12).astype(np.float32)
    cv = ds.cross_validate(x, y, dict(max_depth=3), n_folds=3, num_boost_round=40, early_stopping_rounds=8, refit=False)
    fold, rounds = cv.folds, int(cv.results["rounds"][0])
    for k in range(3):
        for f in range(5):
            assert np.array_equal(np.unique(x[fold != k, f]), np.unique(x[:, f]))
    assert 8 < rounds <= 40
    batch = ds.ForestTrainerBatch().begin(x, y, fold, [dict(max_depth=3, held_out=k) for k in range(3)])
    heaps = []
    for _ in range(rounds):
        batch.step()
        heaps.append([(info.copy(), leaf.copy()) for info, leaf in batch.last_heap])
    for k in range(3):
        train, held = fold != k, fold == k
        single = ds.ForestTrainer().begin(x[train], y[train], x[held], y[held], max_depth=3)
        assert np.array_equal(single.cuts, batch.cuts) and np.array_equal(single.cut_offsets, batch.cut_offsets)
        for round_ in range(rounds):
            single.step()
            info, leaf = single.last_heap
            assert info.shape == heaps[round_][k][0].shape
            assert info.tobytes() == heaps[round_][k][0].tobytes(), (k, round_)
            assert leaf.tobytes() == heaps[round_][k][1].tobytes(), (k, round_)
        margins = batch.margins(k)
        assert margins[train].tobytes() == single.margins().tobytes()
        assert margins[held].tobytes() == single.eval_margins().tobytes()
        assert single.history == batch.history[k] == cv.fold_history[0][k]
        single.close()
    assert any(np.count_nonzero(info[:, 0] == oracle.SPLIT) >= 3 for info, _ in heaps[0])
    batch.close()


# ---- 2. against the oracle, mixed parameters --------------------------------------------------------------------------
# The issue's third model (min_child_weight 0 AND reg_lambda 0) is outside validate_parameters' ranges, which the batch
# must refuse; it is split into the two models that reach either zero: 2 (min_child_weight 0) and 3 (reg_lambda 0).
MIXED = [dict(max_depth=5, held_out=0), dict(max_depth=5, held_out=1),
         dict(max_depth=2, eta=0.3, min_child_weight=0.0, held_out=0),
         dict(max_depth=2, eta=0.3, min_child_weight=0.5, reg_lambda=0.0, held_out=0),
         dict(max_depth=4, min_child_weight=2.0, beta=1.0, held_out=1), dict(max_depth=5, held_out=-1)]
MIXED_ROUNDS = 8


def run_batch(x, y, fold, models, rounds, active_after=None):
    """Steps a batch; per round the heaps, errors and every model's margins / probabilities / gradients."""
    import doppel_speller_amd as ds
    batch = ds.ForestTrainerBatch().begin(x, y, fold, models)
    record = []
    for round_ in range(rounds):
        active = None if active_after is None or round_ < active_after[0] else active_after[1]
        errors = batch.step(active)
        record.append(dict(errors=errors, heaps=[None if h is None else (h[0].copy(), h[1].copy()) for h in batch.last_heap],
                           margins=[batch.margins(m) for m in range(len(models))],
                           probabilities=[batch.probabilities(m) for m in range(len(models))],
                           gradients=[batch.gradients(m) for m in range(len(models))]))
    return batch, record


@pytest.fixture(scope="module")
def mixed():
    import doppel_speller_amd as ds
    x, y = make_data(5003, 17, 41)                      # 17 features: level 0 needs two feature groups
    fold = ds.fold_assignment(None, 2, seed=4, n=5003)
    batch, record = run_batch(x, y, fold, MIXED, MIXED_ROUNDS)
    return x, y, fold, batch, record


def test_double_zero_regularisation_is_refused():
    import doppel_speller_amd as ds
    x, y = make_data(50, 3, 1)
    with pytest.raises(ValueError, match="cannot both be 0"):
        ds.ForestTrainerBatch().begin(x, y, np.arange(50) % 2, [dict(min_child_weight=0, reg_lambda=0)])


def test_mixed_models_match_the_oracle_every_round(mixed):
    x, y, fold, batch, record = mixed
    per_feature = oracle.cuts(x)
    node_bins = oracle.bins(x, per_feature)
    counts = np.array([c.size for c in per_feature])
    assert np.array_equal(batch.bins(), node_bins)
    deep_splits = 0
    for m, given in enumerate(MIXED):
        model = dict(cv_oracle.DEFAULTS, **given)
        held = fold == model["held_out"]
        leafsum = np.zeros(x.shape[0], np.float32)
        for round_, step in enumerate(record):
            p, gh = step["probabilities"][m], step["gradients"][m]
            assert np.array_equal(gh, cv_oracle.zeroed(oracle.gradients(p, y, model["beta"]), fold, model["held_out"]))
            tree, leaves = cv_oracle.grow(node_bins, counts, gh, fold, model)
            heap_equal(step["heaps"][m], tree)
            if model["max_depth"] == 5:
                deep_splits += int(np.count_nonzero(tree["state"][15:31] == oracle.SPLIT))
            leafsum = (leafsum + leaves).astype(np.float32)
            forest = batch.model(m, round_ + 1)
            margins = step["margins"][m]
            assert np.array_equal(margins.view(np.uint32), forest.predict(x, output_margin=True).view(np.uint32))
            assert np.array_equal(margins.view(np.uint32), (np.float32(0.0) + leafsum).view(np.uint32))
            if model["held_out"] >= 0:
                assert step["errors"][m] == oracle.custom_error(forest.predict(x[held]), y[held]), (m, round_)
            else:
                assert step["errors"][m] is None
        assert batch.history[m] == [step["errors"][m] for step in record]
    assert deep_splits > 20                               # the depth-5 models split at level 4


def test_a_capped_grid_changes_no_byte(mixed):
    from doppel_speller_amd import tuning
    x, y, fold, _, record = mixed
    tuning.batch_option("max_blocks", 3)
    try:
        batch, capped = run_batch(x, y, fold, MIXED, MIXED_ROUNDS)
        batch.close()
    finally:
        tuning.batch_option("max_blocks", 0)
    for want, got in zip(record, capped):
        assert want["errors"] == got["errors"]
        for key in ("margins", "probabilities", "gradients"):
            assert all(a.tobytes() == b.tobytes() for a, b in zip(want[key], got[key])), key
        assert all(a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
                   for a, b in zip(want["heaps"], got["heaps"]))


# ---- 3. inactive models ----------------------------------------------------------------------------------------------
def test_an_inactive_model_is_untouched_and_the_others_do_not_see_it(mixed):
    x, y, fold, _, _ = mixed
    active = np.ones(len(MIXED), bool)
    active[2] = False
    batch, record = run_batch(x, y, fold, MIXED, 6, active_after=(3, active))
    assert len(batch.trees[2]) == 3 and len(batch.history[2]) == 3 and len(batch.trees[0]) == 6
    for later in record[3:]:
        assert later["errors"][2] is None
        for key in ("margins", "probabilities", "gradients"):
            assert later[key][2].tobytes() == record[2][key][2].tobytes(), key
        assert later["heaps"][2][0].tobytes() == record[2]["heaps"][2][0].tobytes()
    batch.close()
    others = [model for m, model in enumerate(MIXED) if m != 2]
    without, reference = run_batch(x, y, fold, others, 6)
    without.close()
    for round_ in range(6):
        for at, m in enumerate(m for m in range(len(MIXED)) if m != 2):
            assert record[round_]["errors"][m] == reference[round_]["errors"][at]
            for key in ("margins", "probabilities", "gradients"):
                assert record[round_][key][m].tobytes() == reference[round_][key][at].tobytes(), (key, m)
            assert record[round_]["heaps"][m][0].tobytes() == reference[round_]["heaps"][at][0].tobytes()
            assert record[round_]["heaps"][m][1].tobytes() == reference[round_]["heaps"][at][1].tobytes()


# ---- 6. limits -------------------------------------------------------------------------------------------------------
def check_against_oracle(x, y, fold, models, rounds, only=None):
    """Per chosen model and round: gradients, heap tree, margins and error against the oracle."""
    batch, record = run_batch(x, y, fold, models, rounds)
    per_feature = oracle.cuts(x)
    node_bins = oracle.bins(x, per_feature)
    counts = np.array([c.size for c in per_feature])
    trees = []
    for m in (range(len(models)) if only is None else only):
        model = dict(cv_oracle.DEFAULTS, **models[m])
        held = fold == model["held_out"]
        leafsum, first = np.zeros(x.shape[0], np.float32), len(trees)
        for step in record:
            gh = step["gradients"][m]
            assert np.array_equal(gh, cv_oracle.zeroed(oracle.gradients(step["probabilities"][m], y, model["beta"]), fold,
                                                       model["held_out"]))
            tree, leaves = cv_oracle.grow(node_bins, counts, gh, fold, model)
            heap_equal(step["heaps"][m], tree)
            trees.append(tree)
            leafsum = (leafsum + leaves).astype(np.float32)
            assert np.array_equal(step["margins"][m].view(np.uint32), (np.float32(0.0) + leafsum).view(np.uint32))
            if model["held_out"] >= 0:
                forest = batch.model(m, len(trees) - first)
                assert step["errors"][m] == oracle.custom_error(forest.predict(x[held]), y[held])
            else:
                assert step["errors"][m] is None
    batch.close()
    return trees


def test_limit_96_features_depth_8():
    import doppel_speller_amd as ds
    x, y = oracle.deep_wide_data(3000, 7)
    fold = ds.fold_assignment(None, 2, seed=0, n=3000)
    models = [dict(oracle.DEEP, held_out=0), dict(oracle.DEEP, held_out=1)]
    trees = check_against_oracle(x, y, fold, models, 2)
    assert sum(int(np.count_nonzero(tree["state"][127:255] == oracle.SPLIT)) for tree in trees) > 0   # level 7 splits
    assert all(not np.any(tree["feature"][tree["state"] == oracle.SPLIT] == 95) for tree in trees)   # ties lose


def test_limit_one_row_one_feature_256_models():
    x, y = np.array([[1.5]], np.float32), np.array([1.0], np.float32)
    models = [dict(max_depth=1, eta=0.1 + 0.001 * m, held_out=-1 if m % 2 else 0) for m in range(256)]
    check_against_oracle(x, y, np.zeros(1, np.uint8), models, 2)


def test_limit_255_folds():
    import doppel_speller_amd as ds
    x, y = make_data(600, 6, 3)
    fold = ds.fold_assignment(None, 255, seed=2, n=600)
    assert fold.max() == 254
    models = [dict(max_depth=2, eta=0.3, held_out=k) for k in range(255)]
    check_against_oracle(x, y, fold, models, 2, only=(0, 127, 254))


# ---- 7. C ABI errors -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def library():
    import doppel_speller_amd as ds
    handle = ctypes.CDLL(ds.build_library())
    handle.ds_last_error.restype = ctypes.c_char_p
    handle.ds_trainer_batch_bytes.restype = ctypes.c_int64
    handle.ds_trainer_batch_bytes.argtypes = [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]
    handle.ds_trainer_batch_destroy.restype = None
    handle.ds_trainer_batch_destroy.argtypes = [ctypes.c_void_p]
    return handle


# The argument errors (every limit violated in turn) are refused before any device call: tests/test_tuning_cpu.py runs
# them, with or without a GPU.  What needs the device is the refusal of a batch that does not fit.
def test_a_batch_beyond_the_free_hbm_is_refused(library):
    """The size comes from the formula: 256 models of depth 1 over n x 1 with n chosen so that ds_trainer_batch_bytes is
    four times the card's TOTAL memory, whatever is free at the moment.  The host arrays have that many rows (lazily
    zeroed; create reads the labels and folds, about 0.8 GB, and never the features); nothing is allocated on the
    device."""
    free, total = ctypes.c_int64(0), ctypes.c_int64(0)
    assert library.ds_device_memory(0, ctypes.byref(free), ctypes.byref(total)) == 0
    per_row = library.ds_trainer_batch_bytes(2, 1, 256, 1) - library.ds_trainer_batch_bytes(1, 1, 256, 1)
    assert per_row == 1 + 5 + 256 * 28
    n = min(2 ** 31 - 1, 4 * total.value // per_row)
    needed = library.ds_trainer_batch_bytes(n, 1, 256, 1)
    assert needed > 3 * total.value >= 3 * free.value
    features, labels, fold = np.zeros((n, 1), np.float32), np.zeros(n, np.float32), np.zeros(n, np.uint8)
    params = np.array([[1, 0.1, 1, 1, 5]] * 256, np.float64)
    held_out = np.full(256, -1, np.int32)
    out = ctypes.c_void_p(1)
    status = library.ds_trainer_batch_create(_p(features), ctypes.c_int64(n), 1, _p(np.zeros(1, np.float32)),
                                             _p(np.zeros(2, np.int32)), _p(labels), _p(fold), 1, 256, _p(params),
                                             _p(held_out), 0, ctypes.byref(out))
    error = library.ds_last_error().decode()
    if out.value:
        library.ds_trainer_batch_destroy(out)                   # never reached on a card the formula describes
    assert status == -2 and not out.value                                   # DS_E_HIP
    assert str(needed + 4 * n) in error and "are free" in error, error
