"""ForestTrainer on the GPU against the NumPy restatement of its contract (tests/forest_train_oracle.py): bins,
gradients, every tree, margins, the evaluation error and early stopping, bit for bit."""
import numpy as np
import pytest

import forest_train_oracle as oracle
from forest_train_oracle import make_data

pytestmark = pytest.mark.gpu


def heap_equal(device, expected):
    info, leaf = device
    live = expected["state"] != oracle.ABSENT
    assert np.array_equal(info[:, 0], expected["state"])
    split = expected["state"] == oracle.SPLIT
    assert np.array_equal(info[split, 1], expected["feature"][split])
    assert np.array_equal(info[split, 2], expected["bin"][split])
    assert np.array_equal(info[split, 3], expected["default_left"][split])
    leaves = expected["state"] == oracle.LEAF
    assert np.array_equal(leaf[leaves].view(np.uint32), expected["leaf"][leaves].view(np.uint32))
    return int(live.sum())


def test_device_bins_equal_the_oracle():
    import doppel_speller_amd as ds
    x, y = make_data(5003, 66, 1)
    x[:, 10] = np.random.RandomState(2).randint(0, 255, x.shape[0])     # exactly 255 distinct values
    x[:, 11] = np.random.RandomState(3).randint(0, 256, x.shape[0])     # 256: quantile cuts
    trainer = ds.ForestTrainer().begin(x, y)
    expected = oracle.bins(x, oracle.cuts(x))
    assert np.array_equal(trainer.bins(), expected)


def test_probabilities_and_quantized_gradients():
    import doppel_speller_amd as ds
    x, y = make_data(20000, 12, 4)
    trainer = ds.ForestTrainer().begin(x, y, eta=0.3)
    for _ in range(6):
        before = trainer.margins()
        trainer.step()
        p = trainer.probabilities()
        assert np.allclose(p, oracle.sigmoid32(before), rtol=3e-7, atol=0)   # device expf: <= 2 ulp of NumPy's
        assert np.array_equal(trainer.gradients(), oracle.gradients(p, y, 5.0))


CONFIGS = [  # n, features, depth, lambda, min_child_weight, eta
    (1, 3, 1, 1.0, 1.0, 0.1),
    (9, 6, 3, 1.0, 0.0, 0.3),
    (1000, 66, 5, 1.0, 1.0, 0.1),
    (3000, 20, 2, 0.0, 0.5, 0.3),
    (20000, 10, 6, 0.5, 2.0, 0.2),
    (100000, 66, 5, 1.0, 1.0, 0.1),
]


def check_rounds(trainer, x, y, ex, ey, rounds, depth, eta, mcw, lam, max_bin=256):
    """Grow `rounds` trees on a begun trainer and compare every round with the oracle: the heap tree, the gradients,
    the training and evaluation margins (against the leaf sums and ForestModel.predict, bit for bit) and the
    evaluation error.  Returns the oracle's trees."""
    per_feature = oracle.cuts(x, max_bin)
    node_bins = oracle.bins(x, per_feature)
    counts = np.array([c.size for c in per_feature])
    leafsum = np.zeros(x.shape[0], np.float32)
    trees = []
    for round_ in range(rounds):
        error = trainer.step()
        p = trainer.probabilities()
        gh = trainer.gradients()
        assert np.array_equal(gh, oracle.gradients(p, y, 5.0)), round_
        tree, leaves = oracle.grow_tree(node_bins, counts, gh, depth, eta, mcw, lam)
        heap_equal(trainer.last_heap, tree)
        trees.append(tree)
        leafsum = (leafsum + leaves).astype(np.float32)
        model = trainer.model()
        margins = trainer.margins()
        assert np.array_equal(margins.view(np.uint32), model.predict(x, output_margin=True).view(np.uint32)), round_
        assert np.array_equal(margins.view(np.uint32), (np.float32(0.0) + leafsum).view(np.uint32)), round_
        assert np.array_equal(trainer.eval_margins().view(np.uint32),
                              model.predict(ex, output_margin=True).view(np.uint32)), round_
        assert error == oracle.custom_error(model.predict(ex), ey), round_
    return trees


@pytest.mark.parametrize("n,nf,depth,lam,mcw,eta", CONFIGS)
def test_trees_margins_and_errors_match_the_oracle(n, nf, depth, lam, mcw, eta):
    import doppel_speller_amd as ds
    x, y = make_data(n, nf, n + depth)
    ex, ey = make_data(max(1, n // 3), nf, n + depth + 1)
    trainer = ds.ForestTrainer().begin(x, y, ex, ey, max_depth=depth, eta=eta, min_child_weight=mcw, reg_lambda=lam)
    trees = check_rounds(trainer, x, y, ex, ey, 30, depth, eta, mcw, lam)
    split_rounds = sum(int(np.count_nonzero(tree["state"] != oracle.ABSENT)) > 1 for tree in trees)
    if n >= 1000:
        assert split_rounds == 30                  # the comparison covered real trees, not single leaves


def crafted_early_stopping_set(seed=5):
    """Training: region A (x1 < 0) all positive, region B (x1 >= 0) 99 % positive, for x0 > 0; negatives for x0 <= 0.
    A reaches p > 0.9 in fewer rounds than B.  Evaluation: positives in A (the error falls when A crosses 0.9) and
    negatives in B (it rises when B crosses): the best round lies between."""
    rng = np.random.RandomState(seed)
    x = rng.uniform(-1, 1, (20000, 2)).astype(np.float32)
    y = ((x[:, 0] > 0) & ((x[:, 1] < 0) | (rng.rand(20000) < 0.99))).astype(np.float32)
    ex = np.concatenate([np.column_stack([rng.uniform(0.1, 1, 40), rng.uniform(-1, -0.1, 40)]),
                         np.column_stack([rng.uniform(0.1, 1, 10), rng.uniform(0.1, 1, 10)])]).astype(np.float32)
    ey = np.concatenate([np.ones(40), np.zeros(10)]).astype(np.float32)
    return x, y, ex, ey


def test_early_stopping_picks_the_oracle_best_round():
    import doppel_speller_amd as ds
    x, y, ex, ey = crafted_early_stopping_set()
    stepper = ds.ForestTrainer().begin(x, y, ex, ey, max_depth=2)
    history = []
    for _ in range(150):
        stepper.step()
        history.append(oracle.custom_error(stepper.model().predict(ex), ey))
    assert history == stepper.history
    best = int(np.argmin(history))                 # the first minimum
    assert 0 < best and min(history) < history[0] and max(history[best:]) > min(history), history
    trainer = ds.ForestTrainer()
    model = trainer.fit(x, y, ex, ey, max_depth=2, early_stopping_rounds=10, num_boost_round=150)
    expected_best, stopped = 0, len(history) - 1   # xgboost's rule: the first minimum, stop 10 rounds after it
    for round_, error in enumerate(history):
        if error < history[expected_best]:
            expected_best = round_
        if round_ - expected_best >= 10:
            stopped = round_
            break
    assert trainer.best_iteration == expected_best
    assert model.n_trees == expected_best + 1
    assert len(trainer.trees) == stopped + 1
    assert trainer.history == history[:len(trainer.trees)]
    reference = stepper.model(expected_best + 1)
    for key in ("feature", "threshold", "yes", "no", "missing", "tree_offsets"):
        assert np.array_equal(model.arrays[key], reference.arrays[key]), key


def test_fit_is_deterministic_and_save_load_round_trips(tmp_path):
    import doppel_speller_amd as ds
    x, y = make_data(30000, 66, 8)
    ex, ey = make_data(5000, 66, 9)
    first = ds.ForestTrainer().fit(x, y, ex, ey, num_boost_round=25)
    second = ds.ForestTrainer().fit(x, y, ex, ey, num_boost_round=25)
    for key in ("feature", "threshold", "yes", "no", "missing", "tree_offsets"):
        assert first.arrays[key].tobytes() == second.arrays[key].tobytes(), key
    path = str(tmp_path / "model.npz")
    first.save(path)
    loaded = ds.ForestModel.load(path)
    for key in ("feature", "threshold", "yes", "no", "missing", "tree_offsets"):
        assert loaded.arrays[key].dtype == first.arrays[key].dtype
        assert loaded.arrays[key].tobytes() == first.arrays[key].tobytes(), key
    assert loaded.arrays["base_margin"] == first.arrays["base_margin"] and loaded.n_features == first.n_features
    assert np.array_equal(loaded.predict(ex).view(np.uint32), first.predict(ex).view(np.uint32))
    importance = first.feature_importance()
    assert importance.shape == (66,) and abs(importance.sum() - 1) < 1e-12


def test_trained_model_beats_the_all_negative_answer():
    """The example's flow at small size.  A measured run on one MI355X gave a held-out custom error of 132 against 562
    for answering 'no match' everywhere (0.23).  The bar, half of the all-negative error, leaves a margin of 2x."""
    import doppel_speller_amd as ds
    from doppel_speller_amd import synth
    train = synth.make_workload(5000, 1500, seed=21, query_seed=201)
    evaluation = synth.make_workload(5000, 400, seed=21, query_seed=202)
    held_out = synth.make_workload(5000, 1000, seed=21, query_seed=203)
    x, y = synth.training_pairs(train, 10)
    ex, ey = synth.training_pairs(evaluation, 10)
    hx, hy = synth.training_pairs(held_out, 10)
    model = ds.ForestTrainer().fit(x, y, ex, ey)
    trained = oracle.custom_error(model.predict(hx), hy)
    all_negative = int(hy.sum())
    print("held-out custom error: trained", trained, "all negative", all_negative)
    assert trained < 0.5 * all_negative
    tp, tn, fp, fn = ds.evaluation_error_matrix(model, hx, hy)
    assert tp + tn + fp + fn == hy.shape[0] and tp + fn == all_negative and fn + 5 * fp == trained


@pytest.mark.parametrize("sampling", [{}, dict(subsample=0.5, colsample_bytree=0.6, colsample_bylevel=0.6)],
                         ids=["plain", "sampled"])
def test_a_capped_grid_changes_no_byte(sampling):
    """ds_trainer_step runs the round's kernels under the same grid cap as the batch: with 3 workgroups per grid every
    row kernel (clear, gradient, partition, evaluation) strides over its 5003 rows more than once and the histogram
    kernel takes 3 chunks, at two feature groups on level 0.  No byte of any round may depend on it."""
    import doppel_speller_amd as ds
    from doppel_speller_amd import tuning
    x, y = make_data(5003, 17, 41)
    ex, ey = x[:700], y[:700]

    def run():
        trainer = ds.ForestTrainer().begin(x, y, ex, ey, max_depth=5, **sampling)
        rounds = []
        for _ in range(6):
            error = trainer.step()
            rounds.append((trainer.last_heap[0].tobytes(), trainer.last_heap[1].tobytes(), trainer.margins().tobytes(),
                           trainer.eval_margins().tobytes(), trainer.probabilities().tobytes(),
                           trainer.gradients().tobytes(), error))
        deepest = any(np.any(tree_info[15:31, 0] == oracle.SPLIT) for tree_info in
                      (np.frombuffer(r[0], np.int32).reshape(-1, 4) for r in rounds))
        trainer.close()
        return rounds, deepest

    free, deepest = run()
    assert deepest                                  # level 4 has split: the depth is real
    tuning.batch_option("max_blocks", 3)
    try:
        capped, _ = run()
    finally:
        tuning.batch_option("max_blocks", 0)
    for round_, (a, b) in enumerate(zip(free, capped)):
        for name, one, other in zip(("info", "leaf", "margins", "eval_margins", "probabilities", "gradients", "error"),
                                    a, b):
            assert one == other, (round_, name)
