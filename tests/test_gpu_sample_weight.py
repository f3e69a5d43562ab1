"""Sample weights on the GPU ("Sample weights") against the NumPy restatement of the rule
(tests/forest_weight_oracle.py), bit for bit: every round of ForestTrainer and of ForestTrainerBatch, the identities
"all weights 1 is no weights" and "a row of weight 0 is absent", the device forms, cross-validation, train_model's
kind_weights and the library's own refusals.  Where a round is compared with the oracle, the oracle is handed the
device's float32 probabilities and everything downstream is compared bit for bit.  Every refused input is refused on
the host, before a launch."""
import ctypes

import numpy as np
import pytest

import forest_cv_oracle as cv_oracle
import forest_sampling_oracle as sampling_oracle
import forest_train_oracle as oracle
import forest_weight_oracle as weight_oracle
from forest_train_oracle import make_data

pytestmark = pytest.mark.gpu

MODEL_KEYS = ("feature", "threshold", "yes", "no", "missing", "tree_offsets")
ROUNDS = 8


def heap_equal(device, expected):
    """A device heap (a batch's has the slots of its largest depth) against an oracle heap."""
    info, leaf = device
    slots = expected["state"].shape[0]
    assert not info[slots:, 0].any()
    info, leaf = info[:slots], leaf[:slots]
    assert np.array_equal(info[:, 0], expected["state"])
    split = expected["state"] == oracle.SPLIT
    assert np.array_equal(info[split, 1], expected["feature"][split])
    assert np.array_equal(info[split, 2], expected["bin"][split])
    assert np.array_equal(info[split, 3], expected["default_left"][split])
    leaves = expected["state"] == oracle.LEAF
    assert np.array_equal(leaf[leaves].view(np.uint32), expected["leaf"][leaves].view(np.uint32))


def same_model(a, b):
    return all(a.arrays[key].dtype == b.arrays[key].dtype and a.arrays[key].tobytes() == b.arrays[key].tobytes()
               for key in MODEL_KEYS) and a.arrays["base_margin"] == b.arrays["base_margin"]


def same_heaps(a, b):
    return len(a) == len(b) and all(x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes()
                                    for x, y in zip(a, b))


def bits(a):
    return np.asarray(a).tobytes()


# ---- 1. every round against the oracle ---------------------------------------------------------------------------------
def check_rounds(x, y, weights, ex, ey, rounds, **parameters):
    """Steps a weighted trainer `rounds` times and compares every round with the oracle: the gradients at the device's
    own probabilities, the heap tree grown from those integers, the margins against the leaf sums and
    ForestModel.predict, the unweighted evaluation error.  Returns the device's heaps and the oracle's trees."""
    import doppel_speller_amd as ds
    q = dict(sampling_oracle.DEFAULTS, **parameters)
    trainer = ds.ForestTrainer().begin(x, y, ex, ey, sample_weight=weights, **parameters)
    assert trainer.sample_weight.dtype == np.float32 and np.array_equal(trainer.sample_weight, weights)
    per_feature = oracle.cuts(x)
    node_bins = oracle.bins(x, per_feature)
    assert np.array_equal(trainer.bins(), node_bins)                    # the cuts come from the values alone
    counts = np.array([c.size for c in per_feature])
    leafsum = np.zeros(x.shape[0], np.float32)
    heaps, trees = [], []
    for round_ in range(rounds):
        error = trainer.step()
        p, gh = trainer.probabilities(), trainer.gradients()
        expected = weight_oracle.gradients(p, y, weights, q["beta"])
        expected[~sampling_oracle.row_mask(q["sample_seed"], round_, x.shape[0], q["subsample"])] = 0   # by row number
        assert np.array_equal(gh, expected), round_
        assert not gh[weights == 0].any()
        tree, leaves = oracle.grow_tree(node_bins, counts, gh, q["max_depth"], q["eta"], q["min_child_weight"],
                                        q["reg_lambda"])
        heap_equal(trainer.last_heap, tree)
        heaps.append(trainer.last_heap)
        trees.append(tree)
        leafsum = (leafsum + leaves).astype(np.float32)
        model, margins = trainer.model(), trainer.margins()
        assert bits(margins) == bits(model.predict(x, output_margin=True)), round_
        assert bits(margins) == bits(np.float32(0.0) + leafsum), round_
        assert bits(trainer.eval_margins()) == bits(model.predict(ex, output_margin=True)), round_
        assert error == oracle.custom_error(model.predict(ex), ey), round_            # the reference's feval: no weights
    trainer.close()
    return heaps, trees


# n, features, depth, reg_lambda, min_child_weight, eta: the depths 1 .. 6 and the (min_child_weight, reg_lambda) pairs of
# test_gpu_trainer.CONFIGS, among them (0.5, 0.0) and (0.0, 1.0); n at a wave's edge (63, 64, 65), past the 256-thread
# workgroup (257) and at a non-multiple of either (1000, 5003)
CASES = [(1, 3, 1, 1.0, 1.0, 0.1), (9, 6, 3, 1.0, 0.0, 0.3), (63, 6, 2, 0.0, 0.5, 0.3), (64, 10, 4, 1.0, 1.0, 0.1),
         (65, 10, 5, 1.0, 0.0, 0.3), (257, 12, 6, 0.5, 2.0, 0.2), (1000, 66, 5, 1.0, 1.0, 0.1),
         (5003, 17, 6, 0.5, 2.0, 0.2)]


def case_data(n, nf, depth):
    x, y = make_data(n, nf, n + depth)
    ex, ey = make_data(max(1, n // 3), nf, n + depth + 1)
    return x, y, weight_oracle.draw_weights(n, n + depth + 2), ex, ey


@pytest.mark.parametrize("n,nf,depth,lam,mcw,eta", CASES)
def test_every_round_matches_the_oracle(n, nf, depth, lam, mcw, eta):
    x, y, weights, ex, ey = case_data(n, nf, depth)
    _, trees = check_rounds(x, y, weights, ex, ey, ROUNDS, max_depth=depth, eta=eta, min_child_weight=mcw,
                            reg_lambda=lam)
    if n >= 1000:
        assert all(np.count_nonzero(tree["state"] == oracle.SPLIT) > 1 for tree in trees)   # real trees, not single leaves
        assert len(set(np.unique(weights))) == weight_oracle.WEIGHT_VALUES.shape[0]        # zeros and the large one too


def test_every_round_matches_the_oracle_with_rows_drawn():
    """subsample < 1 with weights (the kSampled gradient kernel of the single trainer): the draw is indexed by the row
    number, whatever the weights."""
    x, y, weights, ex, ey = case_data(1000, 12, 4)
    check_rounds(x, y, weights, ex, ey, ROUNDS, max_depth=4, eta=0.3, subsample=0.5, colsample_bytree=1.0, sample_seed=7)


# ---- 2. ones is none ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [{}, dict(subsample=0.5, colsample_bylevel=0.7, sample_seed=3), "init_model"],
                         ids=["plain", "sampled", "continued"])
def test_all_ones_is_the_call_without_weights(extra):
    import doppel_speller_amd as ds
    x, y = make_data(3000, 12, 21)
    ex, ey = make_data(700, 12, 22)
    parameters = dict(max_depth=4, eta=0.3, num_boost_round=12, early_stopping_rounds=4)
    init = None
    if extra == "init_model":
        init = ds.ForestTrainer().fit(x, y, max_depth=3, eta=0.3, num_boost_round=3)
        extra = dict(init_model=init)
    plain, ones = ds.ForestTrainer(), ds.ForestTrainer()
    a = plain.fit(x, y, ex, ey, **parameters, **extra)
    b = ones.fit(x, y, ex, ey, sample_weight=np.ones(3000), **parameters, **extra)
    assert plain.sample_weight is None and ones.sample_weight.dtype == np.float32
    assert same_model(a, b) and same_model(plain.model(), ones.model())
    assert bits(plain.margins()) == bits(ones.margins()) and bits(plain.eval_margins()) == bits(ones.eval_margins())
    assert bits(plain.gradients()) == bits(ones.gradients())
    assert plain.history == ones.history and plain.best_iteration == ones.best_iteration
    assert plain.initial_error == ones.initial_error and len(plain.history) >= 5
    plain.close()
    ones.close()


# ---- 3. zero is absent, 4. the grid does not matter ------------------------------------------------------------------
def fit_heaps(x, y, weights, rounds, **parameters):
    import doppel_speller_amd as ds
    trainer = ds.ForestTrainer().begin(x, y, **parameters, **({} if weights is None else dict(sample_weight=weights)))
    heaps = []
    for _ in range(rounds):
        trainer.step()
        heaps.append(trainer.last_heap)
    margins = trainer.margins()
    cuts = (trainer.cuts.copy(), trainer.cut_offsets.copy())
    trainer.close()
    return heaps, margins, cuts


def check_zero_is_absent(n, weights):
    """The stacked and permuted matrix of the oracle's identity on the device: the trees and leaf bits of the matrix
    alone, which trains unweighted when `weights` is None (the original rows then weigh 1)."""
    x, y = make_data(n, 10, 50 + n)
    parameters = dict(max_depth=4, eta=0.3, min_child_weight=0.5)
    x2, y2, w2, where = weight_oracle.stacked(x, y, np.ones(n, np.float32) if weights is None else weights, 70 + n)
    alone, margins, cuts = fit_heaps(x, y, weights, 6, **parameters)
    both, margins2, cuts2 = fit_heaps(x2, y2, w2, 6, **parameters)
    assert bits(cuts[0]) == bits(cuts2[0]) and bits(cuts[1]) == bits(cuts2[1])
    assert same_heaps(alone, both)
    assert bits(margins) == bits(margins2[where])
    assert any(np.count_nonzero(info[:, 0] == oracle.SPLIT) >= 3 for info, _ in alone)
    return both


@pytest.mark.parametrize("n", [300, 1000])
def test_rows_of_weight_zero_are_absent(n):
    check_zero_is_absent(n, None)
    check_zero_is_absent(n, weight_oracle.draw_weights(n, 60 + n))


def test_a_capped_grid_changes_no_tree():
    """Cases 1 and 3 at n = 5003 with every row grid capped at ONE workgroup, which then strides over all rows, and
    with the default grid: identical trees (check_rounds compares each with the oracle as well)."""
    from doppel_speller_amd import tuning
    n, nf, depth, lam, mcw, eta = CASES[-1]
    x, y, weights, ex, ey = case_data(n, nf, depth)

    def run():
        heaps, _ = check_rounds(x, y, weights, ex, ey, 4, max_depth=depth, eta=eta, min_child_weight=mcw, reg_lambda=lam)
        return heaps, check_zero_is_absent(5003, None)

    free = run()
    tuning.batch_option("max_blocks", 1)
    try:
        capped = run()
    finally:
        tuning.batch_option("max_blocks", 0)
    assert same_heaps(free[0], capped[0]) and same_heaps(free[1], capped[1])


# ---- 5. the batch ------------------------------------------------------------------------------------------------------
PLAIN = [dict(max_depth=4, eta=0.3, held_out=-1), dict(max_depth=5, min_child_weight=0.5, reg_lambda=0.0, held_out=0),
         dict(max_depth=3, eta=0.2, beta=2.0, held_out=2)]
# subsample < 1 needs reg_lambda > 0: the sampled twin of the second model takes 0.5
SAMPLED = [dict(model, subsample=0.6, sample_seed=11 + m, reg_lambda=max(model.get("reg_lambda", 1.0), 0.5))
           for m, model in enumerate(PLAIN)]


def check_batch(x, y, fold, weights, models, rounds, inactive_after=None, begin=None):
    """Steps a weighted batch and compares every model and round with the oracle on the model's training rows with the
    whole matrix's cuts: gradients (held-out and undrawn rows (0, 0)), heap tree, margins, held-out error.
    inactive_after = (round, model): from that round on the model does not step and must stay as it was."""
    import doppel_speller_amd as ds
    batch = begin() if begin is not None else ds.ForestTrainerBatch().begin(x, y, fold, models, sample_weight=weights)
    per_feature = oracle.cuts(x)
    node_bins = oracle.bins(x, per_feature)
    counts = np.array([c.size for c in per_feature])
    assert np.array_equal(batch.bins(), node_bins)
    given = [dict(sampling_oracle.DEFAULTS, **model) for model in models]
    leafsums = [np.zeros(x.shape[0], np.float32) for _ in models]
    frozen = None
    for round_ in range(rounds):
        active = np.ones(len(models), bool)
        if inactive_after is not None and round_ >= inactive_after[0]:
            active[inactive_after[1]] = False
            if frozen is None:
                m = inactive_after[1]
                frozen = (bits(batch.margins(m)), bits(batch.gradients(m)), bits(batch.probabilities(m)),
                          len(batch.trees[m]))
        errors = batch.step(active)
        for m, model in enumerate(given):
            if not active[m]:
                assert errors[m] is None
                assert frozen == (bits(batch.margins(m)), bits(batch.gradients(m)), bits(batch.probabilities(m)),
                                  len(batch.trees[m]))
                continue
            trains = fold != model["held_out"]
            drawn = np.zeros(x.shape[0], bool)
            drawn[trains] = sampling_oracle.row_mask(model["sample_seed"], round_, int(trains.sum()), model["subsample"])
            gh = batch.gradients(m)
            expected = weight_oracle.gradients(batch.probabilities(m), y, weights, model["beta"])
            expected[~drawn] = 0
            assert np.array_equal(gh, expected), (m, round_)
            tree, leaves = cv_oracle.grow(node_bins, counts, gh, fold, model)
            heap_equal(batch.last_heap[m], tree)
            leafsums[m] = (leafsums[m] + leaves).astype(np.float32)
            assert bits(batch.margins(m)) == bits(np.float32(0.0) + leafsums[m]), (m, round_)
            if model["held_out"] >= 0:
                forest = batch.model(m)
                assert errors[m] == oracle.custom_error(forest.predict(x[~trains]), y[~trains]), (m, round_)
            else:
                assert errors[m] is None
    return batch


@pytest.fixture(scope="module")
def batch_data():
    import doppel_speller_amd as ds
    x, y = make_data(1000, 17, 33)
    return x, y, ds.fold_assignment(None, 3, seed=5, n=1000), weight_oracle.draw_weights(1000, 34)


def test_batch_models_match_the_oracle_every_round(batch_data):
    """Six models over one matrix and one weight array: held_out in {-1, 0, 2}, each with and without subsample = 0.6
    (once a model samples, the step runs the kSampled kernels for all); the second model of the list goes inactive."""
    x, y, fold, weights = batch_data
    batch = check_batch(x, y, fold, weights, PLAIN + SAMPLED, ROUNDS, inactive_after=(3, 1))
    assert len(batch.trees[1]) == 3 and len(batch.trees[0]) == ROUNDS
    assert batch.sample_weight.dtype == np.float32 and np.array_equal(batch.sample_weight, weights)
    batch.close()


def test_unsampled_batch_models_match_the_oracle_every_round(batch_data):
    """The three models without a draw alone: the kFolds gradient kernel without kSampled."""
    x, y, fold, weights = batch_data
    check_batch(x, y, fold, weights, PLAIN, ROUNDS).close()


def test_a_batch_model_without_training_weight_is_refused_by_name(batch_data):
    import doppel_speller_amd as ds
    from doppel_speller_amd import _lib
    x, y, fold, weights = batch_data
    only_fold_2 = np.where(fold == 2, weights + 1, 0).astype(np.float32)          # the model that holds fold 2 out has none
    with pytest.raises(ValueError, match=r"model 2: the total sample weight of its training rows \(outside fold 2\)"):
        ds.ForestTrainerBatch().begin(x, y, fold, PLAIN, sample_weight=only_fold_2)
    batch = ds.ForestTrainerBatch().begin(x, y, fold, PLAIN)                        # the library's own check
    status = _lib.lib().ds_trainer_batch_set_weights(batch.handle, _lib.pointer(only_fold_2))
    message = _lib.lib().ds_last_error().decode()
    assert status == -1 and "model 2: the total weight of its training rows is 0" in message, message
    plain = ds.ForestTrainerBatch().begin(x, y, fold, PLAIN)
    for _ in range(2):                                                              # the refused batch steps unweighted
        assert batch.step() == plain.step()
    assert all(same_heaps([a], [b]) for a, b in zip(batch.last_heap, plain.last_heap))
    batch.close()
    plain.close()


# ---- 6. the device forms -----------------------------------------------------------------------------------------------
def test_device_forms_grow_the_trees_of_the_host_forms(batch_data):
    import doppel_speller_amd as ds
    from doppel_speller_amd import _lib
    x, y, fold, weights = batch_data
    ex, ey = make_data(300, 17, 35)
    parameters = dict(max_depth=4, eta=0.3)
    d_x, d_ex = _lib.DeviceArray.from_host(x), _lib.DeviceArray.from_host(ex)
    try:
        host, device, stepped = ds.ForestTrainer(), ds.ForestTrainer(), ds.ForestTrainer()
        a = host.fit(x, y, ex, ey, sample_weight=weights, num_boost_round=6, **parameters)
        b = device.fit_device(d_x, 1000, y, d_ex, 300, ey, sample_weight=weights, num_boost_round=6, **parameters)
        stepped.begin_device(d_x, 1000, y, d_ex, 300, ey, sample_weight=weights, **parameters)
        for _ in range(6):
            stepped.step()
        assert same_model(a, b) and same_model(host.model(), stepped.model()) and host.history == stepped.history
        assert bits(host.margins()) == bits(device.margins()) == bits(stepped.margins())
        unweighted = ds.ForestTrainer().fit(x, y, ex, ey, num_boost_round=6, **parameters)
        assert not same_model(a, unweighted)                                       # the weights do shape the trees
        for trainer in (host, device, stepped):
            trainer.close()
        on_host = ds.ForestTrainerBatch().begin(x, y, fold, PLAIN, sample_weight=weights)
        in_hbm = check_batch(x, y, fold, weights, PLAIN, 3, begin=lambda: ds.ForestTrainerBatch().begin_device(
            d_x, 1000, y, fold, PLAIN, sample_weight=weights))
        for _ in range(3):
            on_host.step()
        assert all(same_model(on_host.model(m), in_hbm.model(m)) for m in range(len(PLAIN)))
        on_host.close()
        in_hbm.close()
    finally:
        d_x.free()
        d_ex.free()


# ---- 7. cross-validation -----------------------------------------------------------------------------------------------
SETS = [dict(max_depth=3, eta=0.3), dict(max_depth=4, eta=0.2, min_child_weight=0.5)]
CV = dict(n_folds=3, seed=4, num_boost_round=8, early_stopping_rounds=3)


def test_cross_validate_with_all_ones_is_the_call_without_weights(batch_data):
    import doppel_speller_amd as ds
    x, y, _, _ = batch_data
    plain = ds.cross_validate(x, y, SETS, **CV)
    ones = ds.cross_validate(x, y, SETS, **CV, sample_weight=np.ones(1000))
    assert plain.results.equals(ones.results) and plain.history == ones.history
    assert plain.fold_history == ones.fold_history and plain.chosen == ones.chosen
    assert plain.best_iteration == ones.best_iteration and same_model(plain.model, ones.model)


def test_cross_validate_trains_every_fold_and_the_refit_with_the_weights(batch_data):
    import doppel_speller_amd as ds
    x, y, _, weights = batch_data
    cv = ds.cross_validate(x, y, SETS, **CV, sample_weight=weights)
    trainer = ds.ForestTrainer()
    refit = trainer.fit(x, y, sample_weight=weights, num_boost_round=cv.best_iteration + 1, **cv.best_parameters)
    assert same_model(cv.model, refit)
    trainer.close()
    # the fold models: the same batch stepped here equals the oracle in every round, and cross_validate's unweighted
    # out-of-fold errors are this batch's
    models = [dict(one, held_out=k) for one in SETS for k in range(3)]
    rounds = max(int(r) for r in cv.results["rounds"])
    batch = check_batch(x, y, cv.folds, weights, models, rounds)
    for p in range(len(SETS)):
        for k in range(3):
            length = len(cv.fold_history[p][k])
            assert cv.fold_history[p][k] == batch.history[p * 3 + k][:length]
        summed = [sum(batch.history[p * 3 + k][r] for k in range(3)) for r in range(len(cv.history[p]))]
        assert cv.history[p] == summed                                          # integer errors of rows, no weights
    batch.close()


# ---- 8. train_model ---------------------------------------------------------------------------------------------------
def test_train_model_with_kind_weights_is_the_two_step_chain():
    """300 truth titles, 56 train titles, top_n = 20."""
    import doppel_speller_amd as ds
    from doppel_speller_amd import synth
    w = synth.make_workload(300, 56, seed=31, query_seed=32)
    truth, train = synth._to_strings(w.t_flat, w.t_off), synth._to_strings(w.q_flat, w.q_off)
    ids = np.where(w.actual_row >= 0, w.title_id[np.maximum(w.actual_row, 0)], -1)
    data = dict(top_n=20, sample_n=4, seed=9, transform=False)
    fit = dict(num_boost_round=6, early_stopping_rounds=6, max_depth=3, eta=0.3)
    kinds = dict(generated=0.5, positive=2)
    result = ds.train_model(truth, w.title_id, train, ids, **data, **fit, kind_weights=kinds)
    fe = ds.FeatureEngineering(truth, w.title_id, train, ids, **data)
    sets = fe.generate_device_data_sets()
    weights = ds.kind_weights(fe.rows, kinds)
    assert weights.shape == (sets.n_train,) and set(np.unique(weights)) == {0.5, 1.0, 2.0}
    trainer = ds.ForestTrainer()
    chain = trainer.fit_device(sets.train, sets.n_train, sets.train_target, sets.evaluation, sets.n_evaluation,
                               sets.evaluation_target, sample_weight=weights, **fit)
    assert same_model(result.model, chain) and result.history == trainer.history
    assert result.best_iteration == trainer.best_iteration and result.rows.equals(fe.rows)
    trainer.close()
    sets.free()
    plain = ds.train_model(truth, w.title_id, train, ids, **data, **fit)
    ones = ds.train_model(truth, w.title_id, train, ids, **data, **fit,
                          kind_weights=dict(generated=1.0, negative=1.0, positive=1.0))
    assert same_model(plain.model, ones.model) and plain.history == ones.history
    assert plain.error_matrix == ones.error_matrix and not same_model(plain.model, result.model)


# ---- 9. the library refuses on its own -----------------------------------------------------------------------------------
def test_the_library_refuses_bad_weights_and_the_trainer_stays_usable_unweighted():
    import doppel_speller_amd as ds
    from doppel_speller_amd import _lib
    x, y = make_data(257, 6, 90)
    library = _lib.lib()

    def refused(trainer, weights, message):
        status = library.ds_trainer_set_weights(trainer.handle, _lib.pointer(weights))
        text = library.ds_last_error().decode()
        assert status == -1 and message in text, (status, text)                 # DS_E_ARG

    good = weight_oracle.draw_weights(257, 91)
    with_nan, negative = good.copy(), good.copy()
    with_nan[100], negative[256] = np.nan, -0.25
    too_much = np.full(257, 2.0 ** 23, np.float32)          # total 257 * 2^23 > 2^32 / 5
    trainer = ds.ForestTrainer().begin(x, y, max_depth=3)
    refused(trainer, with_nan, "weight 100 is not finite")
    refused(trainer, np.where(np.arange(257) == 7, np.inf, good).astype(np.float32), "weight 7 is not finite")
    refused(trainer, negative, "weight 256 is negative")
    refused(trainer, np.zeros(257, np.float32), "the total weight of the training rows is 0")
    refused(trainer, too_much, "exceeds 2^32")
    refused(trainer, None, "weights is null")
    plain = ds.ForestTrainer().begin(x, y, max_depth=3)
    for _ in range(3):                                     # every refusal left the trainer unweighted and usable
        trainer.step()
        plain.step()
        assert np.array_equal(trainer.gradients(), oracle.gradients(trainer.probabilities(), y, 5.0))
        assert same_heaps([trainer.last_heap], [plain.last_heap])
    refused(trainer, good, "before the first round")        # after a step
    trainer.step()
    plain.step()
    assert same_heaps([trainer.last_heap], [plain.last_heap]) and bits(trainer.margins()) == bits(plain.margins())
    trainer.close()
    plain.close()
    weighted = ds.ForestTrainer().begin(x, y, max_depth=3, sample_weight=good)
    refused(weighted, good, "already set")                  # a second call
    weighted.step()
    assert np.array_equal(weighted.gradients(), weight_oracle.gradients(weighted.probabilities(), y, good, 5.0))
    weighted.close()
    handle = ctypes.c_void_p()                              # before the labels are in
    cuts, offsets = ds.compute_cuts(x)
    _lib.check(library.ds_trainer_create(_lib.pointer(x), 257, 6, _lib.pointer(cuts), _lib.pointer(offsets), 3, 0.1, 1.0,
                                         1.0, 5.0, 0, ctypes.byref(handle)), "ds_trainer_create")
    try:
        assert library.ds_trainer_set_weights(handle, _lib.pointer(good)) == -1
        assert "no labels" in library.ds_last_error().decode()
    finally:
        library.ds_trainer_destroy(handle)
