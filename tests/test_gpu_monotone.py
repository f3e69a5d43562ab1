"""Monotone constraints on the GPU ("Monotone constraints") against the NumPy restatement of the
rule (tests/forest_monotone_oracle.py), bit for bit: every round of ForestTrainer and of ForestTrainerBatch, constraints
that never bind, "all zeros is no constraints" down to the library calls, the compositions with subsampling, sample
weights and init_model, the margin's monotonicity row by row, the device forms, cross-validation, train_model and the
library's own refusals.  Where a round is compared with the oracle, the oracle is handed the device's quantized
gradients (taken at the device's float32 probabilities) and everything downstream is compared bit for bit."""
import ctypes

import numpy as np
import pytest

import forest_monotone_oracle as monotone_oracle
import forest_sampling_oracle as sampling_oracle
import forest_train_oracle as oracle
import forest_weight_oracle as weight_oracle
from forest_train_oracle import make_data

pytestmark = pytest.mark.gpu

MODEL_KEYS = ("feature", "threshold", "yes", "no", "missing", "tree_offsets")
ROUNDS = monotone_oracle.ROUNDS


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


def new_tree_violations(trainer_trees, n_features, constraints):
    """ForestModel's violation count of the trees a trainer has grown itself (without an init model's)."""
    import doppel_speller_amd as ds
    empty = dict(feature=np.zeros(0, np.int32), threshold=np.zeros(0, np.float32), yes=np.zeros(0, np.int32),
                 no=np.zeros(0, np.int32), missing=np.zeros(0, np.int32), tree_offsets=np.zeros(1, np.int64),
                 base_margin=0.0)
    arrays = ds.ForestModel.extended_arrays(empty, trainer_trees)
    return ds.ForestModel.monotone_violations_of(arrays, np.asarray(constraints)[:n_features])


# ---- 1. every round against the oracle ---------------------------------------------------------------------------------
def check_rounds(x, y, constraints, rounds, **parameters):
    """Steps a constrained trainer and compares every round with the oracle: the gradients (untouched by the
    constraints), the heap tree grown from those integers under the constraints, the margins against the leaf sums and
    ForestModel.predict.  Returns the device's heaps, the oracle's trees and the oracle's counts summed over the rounds."""
    import doppel_speller_amd as ds
    q = dict(sampling_oracle.DEFAULTS, **parameters)
    trainer = ds.ForestTrainer().begin(x, y, monotone_constraints=constraints, **parameters)
    assert trainer.monotone_constraints.dtype == np.int8 and np.array_equal(trainer.monotone_constraints, constraints)
    per_feature = oracle.cuts(x)
    node_bins = oracle.bins(x, per_feature)
    assert np.array_equal(trainer.bins(), node_bins)
    counts = np.array([c.size for c in per_feature])
    leafsum = np.zeros(x.shape[0], np.float32)
    heaps, trees, seen = [], [], dict(rejected=0, clamped=0, rejected_at=set())
    for round_ in range(rounds):
        trainer.step()
        gh = trainer.gradients()
        assert np.array_equal(gh, oracle.gradients(trainer.probabilities(), y, q["beta"])), round_
        tree, leaves, counted = monotone_oracle.grow_tree(node_bins, counts, gh, constraints, q["max_depth"], q["eta"],
                                                          q["min_child_weight"], q["reg_lambda"])
        heap_equal(trainer.last_heap, tree)
        heaps.append(trainer.last_heap)
        trees.append(tree)
        seen["rejected"] += counted["rejected"]
        seen["clamped"] += counted["clamped"]
        seen["rejected_at"] |= set(counted["rejected_at"])
        leafsum = (leafsum + leaves).astype(np.float32)
        model, margins = trainer.model(), trainer.margins()
        assert bits(margins) == bits(model.predict(x, output_margin=True)), round_
        assert bits(margins) == bits(np.float32(0.0) + leafsum), round_
        assert monotone_oracle.violations(tree, constraints) == 0, round_
    assert trainer.model().monotone_violations(constraints) == 0
    trainer.close()
    return heaps, trees, seen


def fit_heaps(x, y, rounds, **arguments):
    import doppel_speller_amd as ds
    trainer = ds.ForestTrainer().begin(x, y, **arguments)
    heaps = []
    for _ in range(rounds):
        trainer.step()
        heaps.append(trainer.last_heap)
    margins = trainer.margins()
    trainer.close()
    return heaps, margins


@pytest.mark.parametrize("n,nf,depth,lam,mcw,eta", [monotone_oracle.ONE_ROW] + monotone_oracle.CASES)
def test_every_round_matches_the_oracle(n, nf, depth, lam, mcw, eta):
    x, y = make_data(n, nf, 5)
    constraints = monotone_oracle.case_constraints(nf)
    config = dict(max_depth=depth, eta=eta, min_child_weight=mcw, reg_lambda=lam)
    heaps, trees, seen = check_rounds(x, y, constraints, ROUNDS, **config)
    free, _ = fit_heaps(x, y, ROUNDS, **config)
    if n == 1:
        assert same_heaps(heaps, free) and seen["rejected"] == 0          # one row: the root leaf either way
        return
    assert seen["rejected"] > 0                                           # the constraints bound what the device grew
    assert not any(same_heaps([a], [b]) for a, b in zip(heaps, free))     # all four trees differ from the free ones
    if n in monotone_oracle.CLAMPING:
        assert seen["clamped"] >= 1


def test_every_round_matches_the_oracle_at_depth_8_and_96_features():
    """DEEP on deep_wide_data(6000): column 95 copies column 0 and is constrained the other way, so of every tied pair
    of candidates one is rejected; the second split workgroup of level 7 (heap ids 191 .. 254) sees rejections too."""
    x, y = oracle.deep_wide_data(6000)
    constraints = np.zeros(96, np.int8)
    constraints[0], constraints[2], constraints[95] = 1, 1, -1
    _, trees, seen = check_rounds(x, y, constraints, 3, **oracle.DEEP)
    assert seen["rejected"] > 0 and seen["clamped"] > 0
    assert any(191 <= node < 255 for node in seen["rejected_at"])
    assert any(oracle.deep_paths(tree)[1] > 0 and oracle.deep_paths(tree)[2] > 0 for tree in trees)
    assert any((tree["feature"][tree["state"] == oracle.SPLIT] == 0).any() for tree in trees)


# ---- 2. constraints that never bind, all zeros, None ---------------------------------------------------------------------
@pytest.mark.parametrize("n,nf,depth,lam,mcw,eta", monotone_oracle.CASES[1:3] + monotone_oracle.CASES[-1:])
def test_constraints_that_never_bind_grow_the_unconstrained_trees(n, nf, depth, lam, mcw, eta):
    """Constraints on the constant column 3 and the all-NaN column 4 alone run the kMonotone kernels, whose every number
    equals the plain kernels' while no bound is finite."""
    x, y = make_data(n, nf, 5)
    config = dict(max_depth=depth, eta=eta, min_child_weight=mcw, reg_lambda=lam)
    idle = monotone_oracle.idle_constraints(nf)
    assert idle.any()
    plain, plain_margins = fit_heaps(x, y, ROUNDS, **config)
    bound, bound_margins = fit_heaps(x, y, ROUNDS, monotone_constraints=idle, **config)
    assert same_heaps(plain, bound) and bits(plain_margins) == bits(bound_margins)


class _Recorder:
    """The library with the name of every entry called through it written down."""

    def __init__(self, library):
        self._library, self.calls = library, []

    def __getattr__(self, name):
        entry = getattr(self._library, name)
        if not callable(entry):
            return entry

        def call(*arguments):
            self.calls.append(name)
            return entry(*arguments)
        return call


@pytest.mark.parametrize("extra", [{}, dict(subsample=0.5, colsample_bylevel=0.7, sample_seed=3), "sample_weight",
                                   "init_model"], ids=["plain", "sampled", "weighted", "continued"])
def test_all_zeros_and_none_make_todays_library_calls(monkeypatch, extra):
    import doppel_speller_amd as ds
    from doppel_speller_amd import _lib
    x, y = make_data(1000, 10, 21)
    ex, ey = make_data(300, 10, 22)
    parameters = dict(max_depth=4, eta=0.3, num_boost_round=6, early_stopping_rounds=6)
    if extra == "init_model":
        extra = dict(init_model=ds.ForestTrainer().fit(x, y, max_depth=3, eta=0.3, num_boost_round=2))
    elif extra == "sample_weight":
        extra = dict(sample_weight=weight_oracle.draw_weights(1000, 23))
    fold = ds.fold_assignment(None, 3, seed=5, n=1000)
    batch_models = [dict(max_depth=3, held_out=0), dict(max_depth=4, held_out=-1)]
    batch_extra = {k: v for k, v in extra.items() if k in ("init_model", "sample_weight")}
    if "subsample" in extra:
        batch_models = [dict(model, subsample=0.5, sample_seed=3) for model in batch_models]
    recorder = _Recorder(_lib.lib())
    monkeypatch.setattr(_lib, "lib", lambda: recorder)
    runs = []
    for constraints in ({}, dict(monotone_constraints=None), dict(monotone_constraints=np.zeros(10, np.int8)),
                        dict(monotone_constraints=[0] * 10)):
        recorder.calls = []
        trainer = ds.ForestTrainer()
        model = trainer.fit(x, y, ex, ey, **parameters, **extra, **constraints)
        batch = ds.ForestTrainerBatch().begin(x, y, fold, batch_models, **batch_extra, **constraints)
        errors = [batch.step() for _ in range(3)]
        runs.append(([name for name in recorder.calls if not name.endswith("_destroy") and name != "ds_free"], model, trainer.history, bits(trainer.margins()), errors,
                     [bits(batch.margins(m)) for m in range(2)]))
        expected = None if constraints.get("monotone_constraints") is None else np.zeros(10, np.int8)
        for holder in (trainer, batch):
            kept = holder.monotone_constraints
            assert kept is None if expected is None else (kept.dtype == np.int8 and np.array_equal(kept, expected))
        trainer.close()
        batch.close()
    first = runs[0]
    assert "ds_trainer_step" in first[0] and "ds_trainer_batch_step" in first[0]
    for run in runs:
        assert not any("monotone" in name for name in run[0])
        assert run[0] == first[0]                                 # the same entries in the same order (frees aside)
        assert same_model(run[1], first[1]) and run[2:] == first[2:]


# ---- 3. composition ----------------------------------------------------------------------------------------------------
COMPOSED = dict(max_depth=5, eta=0.3, min_child_weight=0.5)


@pytest.fixture(scope="module")
def composed_data():
    x, y = make_data(2000, 10, 41)
    return x, y, monotone_oracle.case_constraints(10)


@pytest.mark.parametrize("extra", [dict(subsample=0.5, colsample_bylevel=0.7, sample_seed=3), "sample_weight",
                                   "init_model"], ids=["sampled", "weighted", "continued"])
def test_constrained_training_composes(composed_data, extra):
    """With row and column draws, with sample weights and after an (unconstrained) init model the new trees have no
    violation, and they are not the trees of the same call without constraints, which has some."""
    import doppel_speller_amd as ds
    x, y, constraints = composed_data
    if extra == "init_model":
        extra = dict(init_model=ds.ForestTrainer().fit(x, y, max_depth=4, eta=0.3, num_boost_round=3))
        assert extra["init_model"].monotone_violations(constraints) > 0          # the init trees are what they are
    elif extra == "sample_weight":
        extra = dict(sample_weight=weight_oracle.draw_weights(2000, 42))
    bound, free = ds.ForestTrainer(), ds.ForestTrainer()
    bound.fit(x, y, num_boost_round=6, monotone_constraints=constraints, **COMPOSED, **extra)
    free.fit(x, y, num_boost_round=6, **COMPOSED, **extra)
    assert len(bound.trees) == 6
    assert new_tree_violations(bound.trees, 10, constraints) == 0
    assert new_tree_violations(free.trees, 10, constraints) > 0
    if "init_model" in extra:                                # the whole forest keeps exactly the init trees' violations
        assert bound.model().monotone_violations(constraints) == extra["init_model"].monotone_violations(constraints)
    bound.close()
    free.close()


@pytest.mark.parametrize("sampling", [{}, dict(subsample=0.6, colsample_bytree=0.8, sample_seed=9)],
                         ids=["plain", "sampled"])
def test_k_rounds_continued_for_m_more_are_k_plus_m_rounds(composed_data, sampling):
    import doppel_speller_amd as ds
    x, y, constraints = composed_data
    arguments = dict(COMPOSED, monotone_constraints=constraints, **sampling)
    straight = ds.ForestTrainer().fit(x, y, num_boost_round=7, **arguments)
    head = ds.ForestTrainer().fit(x, y, num_boost_round=3, **arguments)
    trainer = ds.ForestTrainer()
    continued = trainer.fit(x, y, num_boost_round=4, init_model=head, **arguments)
    assert same_model(straight, continued) and straight.monotone_violations(constraints) == 0
    assert same_model(straight.head(3), head) and len(trainer.trees) == 4
    trainer.close()


# ---- 4. the margin itself is monotone ------------------------------------------------------------------------------------
def test_the_margin_is_monotone_in_every_constrained_feature(composed_data):
    """64 rows, one constrained feature swept over all its cuts (and a value below the first) while the others are
    held: the margin never decreases for +1 and never increases for -1.  The unconstrained model breaks it."""
    import doppel_speller_amd as ds
    x, y, constraints = composed_data
    trainer, free = ds.ForestTrainer(), ds.ForestTrainer()
    model = trainer.fit(x, y, num_boost_round=8, monotone_constraints=constraints, **COMPOSED)
    plain = free.fit(x, y, num_boost_round=8, **COMPOSED)
    broken = moved = 0
    for f in np.nonzero(constraints)[0]:
        cuts = trainer.cuts[trainer.cut_offsets[f]:trainer.cut_offsets[f + 1]]
        values = np.concatenate(([cuts[0] - np.float32(1.0)], cuts)).astype(np.float32)
        assert values.shape[0] >= 4 and (np.diff(values) > 0).all()
        rows = np.repeat(x[:64], values.shape[0], axis=0)
        rows[:, f] = np.tile(values, 64)
        steps = np.diff(model.predict(rows, output_margin=True).reshape(64, -1), axis=1) * constraints[f]
        assert (steps >= 0).all(), f
        moved += int((steps > 0).any())
        broken += int((np.diff(plain.predict(rows, output_margin=True).reshape(64, -1), axis=1) * constraints[f] < 0).any())
    assert broken >= 1 and moved >= 1                 # column 0, constrained against its signal, may well never split
    trainer.close()
    free.close()


# ---- 5. the grid does not matter -----------------------------------------------------------------------------------------
def test_a_capped_grid_changes_no_tree():
    from doppel_speller_amd import tuning
    n, nf, depth, lam, mcw, eta = monotone_oracle.CASES[-1]
    x, y = make_data(n, nf, 5)
    arguments = dict(max_depth=depth, eta=eta, min_child_weight=mcw, reg_lambda=lam,
                     monotone_constraints=monotone_oracle.case_constraints(nf))
    free = fit_heaps(x, y, ROUNDS, **arguments)
    tuning.batch_option("max_blocks", 2)
    try:
        capped = fit_heaps(x, y, ROUNDS, **arguments)
    finally:
        tuning.batch_option("max_blocks", 0)
    assert same_heaps(free[0], capped[0]) and bits(free[1]) == bits(capped[1])


# ---- 6. the batch ------------------------------------------------------------------------------------------------------
MODELS = [dict(max_depth=4, eta=0.3, held_out=-1), dict(max_depth=6, min_child_weight=0.5, reg_lambda=0.0, held_out=0),
          dict(max_depth=2, eta=0.2, reg_lambda=2.0, held_out=2),
          dict(max_depth=5, eta=0.3, reg_lambda=0.5, held_out=1, subsample=0.6, sample_seed=11)]


def check_batch(x, y, fold, constraints, models, rounds, begin=None):
    """Steps a constrained batch and compares every model and round with the oracle on the model's training rows with
    the whole matrix's cuts: gradients (held-out and undrawn rows (0, 0)), heap tree, margins, held-out error."""
    import doppel_speller_amd as ds
    batch = begin() if begin is not None else ds.ForestTrainerBatch().begin(x, y, fold, models,
                                                                             monotone_constraints=constraints)
    per_feature = oracle.cuts(x)
    node_bins = oracle.bins(x, per_feature)
    counts = np.array([c.size for c in per_feature])
    given = [dict(sampling_oracle.DEFAULTS, **model) for model in models]
    leafsums = [np.zeros(x.shape[0], np.float32) for _ in models]
    rejected = [0] * len(models)
    for round_ in range(rounds):
        errors = batch.step()
        for m, model in enumerate(given):
            trains = fold != model["held_out"]
            drawn = np.zeros(x.shape[0], bool)
            drawn[trains] = sampling_oracle.row_mask(model["sample_seed"], round_, int(trains.sum()), model["subsample"])
            gh = batch.gradients(m)
            expected = oracle.gradients(batch.probabilities(m), y, model["beta"])
            expected[~drawn] = 0
            assert np.array_equal(gh, expected), (m, round_)
            tree, leaves, counted = monotone_oracle.grow_tree(node_bins, counts, gh, constraints, model["max_depth"],
                                                              model["eta"], model["min_child_weight"],
                                                              model["reg_lambda"])
            heap_equal(batch.last_heap[m], tree)
            rejected[m] += counted["rejected"]
            leafsums[m] = (leafsums[m] + leaves).astype(np.float32)
            assert bits(batch.margins(m)) == bits(np.float32(0.0) + leafsums[m]), (m, round_)
            if model["held_out"] >= 0:
                assert errors[m] == oracle.custom_error(batch.model(m).predict(x[~trains]), y[~trains]), (m, round_)
            else:
                assert errors[m] is None
    assert all(count > 0 for count in rejected)
    assert all(batch.model(m).monotone_violations(constraints) == 0 for m in range(len(models)))
    return batch


@pytest.fixture(scope="module")
def batch_data():
    import doppel_speller_amd as ds
    x, y = make_data(1000, 10, 33)
    return x, y, ds.fold_assignment(None, 3, seed=5, n=1000), monotone_oracle.case_constraints(10)


def test_batch_models_match_the_oracle_every_round_on_host_and_device_forms(batch_data):
    """Three models of different depth, lambda and held-out fold and one that draws rows, over one matrix and ONE
    constraint vector (once a model samples, the step runs the kSampled kernels for all)."""
    import doppel_speller_amd as ds
    from doppel_speller_amd import _lib
    x, y, fold, constraints = batch_data
    on_host = check_batch(x, y, fold, constraints, MODELS, ROUNDS)
    assert on_host.monotone_constraints.dtype == np.int8 and np.array_equal(on_host.monotone_constraints, constraints)
    d_x = _lib.DeviceArray.from_host(x)
    try:
        in_hbm = ds.ForestTrainerBatch().begin_device(d_x, 1000, y, fold, MODELS, monotone_constraints=constraints)
        for _ in range(ROUNDS):
            in_hbm.step()
        assert all(same_model(on_host.model(m), in_hbm.model(m)) for m in range(len(MODELS)))
        assert on_host.history == in_hbm.history
        in_hbm.close()
        plain = [model for model in MODELS if "subsample" not in model]           # the kernels without kSampled
        check_batch(x, y, fold, constraints, plain, 2).close()
        trainer = ds.ForestTrainer()                                               # and the single trainer's device forms
        a = trainer.fit_device(d_x, 1000, y, num_boost_round=ROUNDS, monotone_constraints=constraints,
                               **{k: v for k, v in MODELS[0].items() if k != "held_out"})
        assert same_model(a, on_host.model(0))
        trainer.close()
    finally:
        d_x.free()
        on_host.close()


# ---- 7. cross-validation -----------------------------------------------------------------------------------------------
SETS = [dict(max_depth=3, eta=0.3), dict(max_depth=4, eta=0.2, min_child_weight=0.5)]
CV = dict(n_folds=3, seed=4, num_boost_round=6, early_stopping_rounds=3)


def test_cross_validate_constrains_every_fold_and_the_refit(batch_data):
    import doppel_speller_amd as ds
    x, y, _, constraints = batch_data
    cv = ds.cross_validate(x, y, SETS, **CV, monotone_constraints=constraints)
    trainer = ds.ForestTrainer()
    refit = trainer.fit(x, y, monotone_constraints=constraints, num_boost_round=cv.best_iteration + 1,
                        **cv.best_parameters)
    assert same_model(cv.model, refit) and cv.model.monotone_violations(constraints) == 0
    trainer.close()
    free = ds.cross_validate(x, y, SETS, **CV)
    assert free.model.monotone_violations(constraints) > 0 and not same_model(cv.model, free.model)
    # the fold models: the same batch stepped here equals the oracle in every round (check_batch), and
    # cross_validate's out-of-fold errors are this batch's
    models = [dict(one, held_out=k) for one in SETS for k in range(3)]
    rounds = max(int(r) for r in cv.results["rounds"])
    batch = check_batch(x, y, cv.folds, constraints, models, rounds)
    for p in range(len(SETS)):
        for k in range(3):
            length = len(cv.fold_history[p][k])
            assert cv.fold_history[p][k] == batch.history[p * 3 + k][:length]
    batch.close()


# ---- 8. train_model ---------------------------------------------------------------------------------------------------
def test_train_model_with_ratio_constraints_is_the_two_step_chain():
    """300 truth titles, 56 train titles, top_n = 20."""
    import doppel_speller_amd as ds
    from doppel_speller_amd import synth
    w = synth.make_workload(300, 56, seed=31, query_seed=32)
    truth, train = synth._to_strings(w.t_flat, w.t_off), synth._to_strings(w.q_flat, w.q_off)
    ids = np.where(w.actual_row >= 0, w.title_id[np.maximum(w.actual_row, 0)], -1)
    data = dict(top_n=20, sample_n=4, seed=9, transform=False)
    fit = dict(num_boost_round=6, early_stopping_rounds=6, max_depth=3, eta=0.3)
    result = ds.train_model(truth, w.title_id, train, ids, **data, **fit, monotone_constraints=ds.ratio_constraints())
    vector = ds.validate_monotone_constraints(ds.ratio_constraints(), ds.FEATURES_COUNT, ds.FEATURE_NAMES)
    fe = ds.FeatureEngineering(truth, w.title_id, train, ids, **data)
    sets = fe.generate_device_data_sets()
    trainer = ds.ForestTrainer()
    chain = trainer.fit_device(sets.train, sets.n_train, sets.train_target, sets.evaluation, sets.n_evaluation,
                               sets.evaluation_target, monotone_constraints=vector, **fit)
    assert same_model(result.model, chain) and result.history == trainer.history
    assert result.best_iteration == trainer.best_iteration and result.rows.equals(fe.rows)
    assert result.model.monotone_violations(vector) == 0 and result.model.n_trees >= 1
    trainer.close()
    sets.free()
    zeros = ds.train_model(truth, w.title_id, train, ids, **data, **fit, monotone_constraints={})
    plain = ds.train_model(truth, w.title_id, train, ids, **data, **fit)
    assert same_model(plain.model, zeros.model) and plain.error_matrix == zeros.error_matrix


# ---- 9. the library refuses on its own -----------------------------------------------------------------------------------
def test_the_library_refuses_bad_vectors_and_the_trainer_stays_usable_unconstrained():
    import doppel_speller_amd as ds
    from doppel_speller_amd import _lib
    x, y = make_data(257, 6, 90)
    library = _lib.lib()
    good = monotone_oracle.case_constraints(6)

    def refused(entry, handle, constraints, message):
        status = getattr(library, entry)(handle, _lib.pointer(constraints))
        text = library.ds_last_error().decode()
        assert status == -1 and message in text, (status, text)                 # DS_E_ARG

    two, minus_two = good.copy(), good.copy()
    two[5], minus_two[3] = 2, -2
    trainer = ds.ForestTrainer().begin(x, y, max_depth=3)
    refused("ds_trainer_set_monotone", trainer.handle, two, "constraint 2 of feature 5 is not -1, 0 or 1")
    refused("ds_trainer_set_monotone", trainer.handle, minus_two, "constraint -2 of feature 3 is not -1, 0 or 1")
    refused("ds_trainer_set_monotone", trainer.handle, None, "constraints is null")
    plain = ds.ForestTrainer().begin(x, y, max_depth=3)
    for _ in range(2):                                     # every refusal left the trainer unconstrained and usable
        trainer.step()
        plain.step()
        assert same_heaps([trainer.last_heap], [plain.last_heap])
    refused("ds_trainer_set_monotone", trainer.handle, good, "before the first round")      # after a step
    trainer.step()
    plain.step()
    assert same_heaps([trainer.last_heap], [plain.last_heap]) and bits(trainer.margins()) == bits(plain.margins())
    trainer.close()
    bound = ds.ForestTrainer().begin(x, y, max_depth=3, monotone_constraints=good)
    refused("ds_trainer_set_monotone", bound.handle, good, "already set")                   # a second call
    bound.step()
    plain_heap = plain.trees[0]
    assert bound.model().monotone_violations(good) == 0 and not np.array_equal(bound.trees[0]["threshold"],
                                                                                plain_heap["threshold"])
    bound.close()
    zeros = ds.ForestTrainer().begin(x, y, max_depth=3)                                      # all zeros: accepted, once
    assert library.ds_trainer_set_monotone(zeros.handle, _lib.pointer(np.zeros(6, np.int8))) == 0
    refused("ds_trainer_set_monotone", zeros.handle, good, "already set")
    zeros.step()
    assert np.array_equal(zeros.trees[0]["threshold"], plain_heap["threshold"])
    zeros.close()
    plain.close()
    handle = ctypes.c_void_p()                              # before the labels are in
    cuts, offsets = ds.compute_cuts(x)
    _lib.check(library.ds_trainer_create(_lib.pointer(x), 257, 6, _lib.pointer(cuts), _lib.pointer(offsets), 3, 0.1, 1.0,
                                         1.0, 5.0, 0, ctypes.byref(handle)), "ds_trainer_create")
    try:
        assert library.ds_trainer_set_monotone(handle, _lib.pointer(good)) == -1
        assert "no labels" in library.ds_last_error().decode()
    finally:
        library.ds_trainer_destroy(handle)
    # the batch's entry
    fold = ds.fold_assignment(None, 3, seed=5, n=257)
    models = [dict(max_depth=3, held_out=0), dict(max_depth=2, held_out=-1)]
    batch, free = ds.ForestTrainerBatch().begin(x, y, fold, models), ds.ForestTrainerBatch().begin(x, y, fold, models)
    refused("ds_trainer_batch_set_monotone", batch.handle, two, "constraint 2 of feature 5 is not -1, 0 or 1")
    refused("ds_trainer_batch_set_monotone", batch.handle, None, "constraints is null")
    assert batch.step() == free.step() and same_heaps(batch.last_heap, free.last_heap)
    refused("ds_trainer_batch_set_monotone", batch.handle, good, "before the first step")
    assert batch.step() == free.step() and same_heaps(batch.last_heap, free.last_heap)
    batch.close()
    free.close()
    bound = ds.ForestTrainerBatch().begin(x, y, fold, models, monotone_constraints=good)
    refused("ds_trainer_batch_set_monotone", bound.handle, good, "already set")
    bound.step()
    assert all(bound.model(m).monotone_violations(good) == 0 for m in range(2))
    bound.close()
