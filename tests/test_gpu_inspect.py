"""Model inspection on the GPU ("Model inspection"; csrc/ds_inspect.hip) against the NumPy
restatement of the rule (tests/forest_inspect_oracle.py).  Everything is integers, so everything is compared exactly:
the five counters of every job of every case in every launch form, the baseline against predict, permutation
importance and partial dependence against the oracle's derived arrays, the partial dependence of a model trained
under monotone constraints, and train_model's permutation importance against the host call."""
import numpy as np
import pytest

import forest_inspect_oracle as oracle
import inspect_cases as cases

pytestmark = pytest.mark.gpu


def model_of(forest, n_features):
    import doppel_speller_amd as ds
    return ds.ForestModel(forest["feature"], forest["threshold"], forest["yes"], forest["no"], forest["missing"],
                          forest["tree_offsets"], n_features, forest["base_margin"])


def job_table(jobs):
    from doppel_speller_amd.forest import inspection_jobs
    return inspection_jobs(jobs)


def fixed_point_sum(margins):
    wide = margins.astype(np.float64)
    return int(np.where(np.isnan(wide), 0.0, np.rint(np.clip(wide, -2048.0, 2048.0) * (1 << 20))).astype(np.int64).sum())


# ---- 1. every case in every launch form ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.NAMES)
def test_counters_equal_the_oracle_in_every_form(name):
    from doppel_speller_amd import _lib
    case = cases.case(name)
    model = model_of(case["forest"], case["n_features"])
    jobs, rows, target, n = job_table(case["jobs"]), case["rows"], case["target"], case["rows"].shape[0]
    d_rows = _lib.DeviceArray.from_host(rows)
    d_target = None if target is None else _lib.DeviceArray.from_host(target)
    runs = [("host", model.inspect(rows, target, jobs, case["seed"], cases.THRESHOLD)),
            ("device", model.inspect_device(d_rows, n, d_target, jobs, case["seed"], cases.THRESHOLD))]
    for option, value in (("max_blocks", 1), ("inspect_jobs_per_block", 1), ("inspect_jobs_per_block", 7),
                          ("inspect_jobs_per_block", len(case["jobs"]) + 5)):
        model.option(option, value)
        runs.append((f"{option}={value}", model.inspect_device(d_rows, n, d_target, jobs, case["seed"], cases.THRESHOLD)))
        model.option(option, 0)
    for form, counters in runs:
        assert counters.dtype == np.uint64 and counters.shape == case["expected"].shape, form
        wrong = np.flatnonzero((counters != case["expected"]).any(axis=1))
        assert wrong.shape[0] == 0, (form, wrong[:5], counters[wrong[:5]], case["expected"][wrong[:5]])
        assert counters.tobytes() == runs[0][1].tobytes(), form
    d_rows.free()
    if d_target is not None:
        d_target.free()
    model.close()


def test_empty_calls_and_refusals_with_a_forest():
    import ctypes
    from doppel_speller_amd import _lib
    case = cases.case("two_rows")
    model = model_of(case["forest"], 7)
    library = _lib.lib()
    rows, out = case["rows"], np.full((3, 5), 9, np.uint64)
    jobs = job_table([(0, 0, 0.0, 0), (1, 6, 0.0, 0), (2, 6, 1.0, 0)])

    def call(jobs_=jobs, n=2, n_jobs=3):
        return library.ds_forest_inspect(model.handle, _lib.pointer(rows), n, None, _lib.pointer(jobs_), n_jobs, 1, 0.9,
                                         _lib.pointer(out))
    assert call(n=0) == 0 and not out.any()                          # no rows: the counters are zeroed
    out[:] = 9
    assert call(n_jobs=0) == 0 and (out == 9).all()                  # no jobs: nothing to zero
    for bad, message in (((1, 7, 0.0, 0), b"feature 7 outside [0, 7)"), ((2, 7, 0.0, 0), b"feature 7 outside [0, 7)"),
                         ((4, 0, 0.0, 0), b"unknown kind 4")):
        table = jobs.copy()
        table[2] = bad
        assert call(jobs_=table) == -1 and message in library.ds_last_error()
        d_rows, d_jobs = _lib.DeviceArray.from_host(rows), _lib.DeviceArray.from_host(table)
        d_out = _lib.DeviceArray.from_host(out)
        assert library.ds_forest_inspect_device(model.handle, d_rows.ptr, 2, None, d_jobs.ptr, 3, 1, 0.9, d_out.ptr,
                                                None) == -1
        assert message in library.ds_last_error() and (d_out.to_host() == 9).all()
    assert (out == 9).all()
    with pytest.raises(_lib.DoppelError, match="inspect_jobs_per_block"):
        model.option("inspect_jobs_per_block", -1)
    model.close()


# ---- 2. the baseline is predict -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["one_workgroup", "three_row_blocks", "base_margin"])
def test_baseline_equals_predict(name):
    from doppel_speller_amd import train
    case = cases.case(name)
    model = model_of(case["forest"], case["n_features"])
    rows, n = case["rows"], case["rows"].shape[0]
    target = np.zeros(n, np.float32) if case["target"] is None else case["target"]
    counters = model.inspect(rows, target, job_table([(0, 0, 0.0, 0)]), 0, 0.9)
    assert tuple(int(v) for v in counters[0, :4]) == train._error_matrix(model.predict(rows), target, 0.9)
    margins = model.predict(rows, output_margin=True)
    assert int(counters[0, 4:5].view(np.int64)[0]) == fixed_point_sum(margins)
    assert margins.tobytes() == oracle.margins(case["forest"], rows).tobytes()
    model.close()


def test_jobs_that_change_nothing_reproduce_the_baseline():
    one = cases.case("one_row")
    model = model_of(one["forest"], 1)
    counters = model.inspect(one["rows"], one["target"], job_table([(0, 0, 0.0, 0), (1, 0, 0.0, 0), (1, 0, 0.0, 3)]), 5)
    assert (counters[1:] == counters[0]).all() and counters[0, :4].sum() == 1
    model.close()
    case = cases.case("stumps")
    rows = np.ascontiguousarray(case["rows"])
    rows[:, 9] = np.float32(42.5)
    rows[:, 10] = np.nan
    model = model_of(case["forest"], 66)
    jobs = [(0, 0, 0.0, 0), (2, 9, np.float32(42.5), 0), (2, 10, np.float32(np.nan), 0), (1, 9, 0.0, 1), (1, 10, 0.0, 2)]
    counters = model.inspect(rows, case["target"], job_table(jobs), 5)
    assert (counters[1:] == counters[0]).all() and counters[0, :4].sum() == rows.shape[0]
    model.close()


# ---- 3. permutation importance and partial dependence ---------------------------------------------------------------------------
def test_permutation_importance_equals_the_oracle():
    case = cases.case("one_workgroup")
    forest, rows, target = case["forest"], case["rows"], case["target"]
    model = model_of(forest, 66)
    unused = sorted(set(range(66)) - set(forest["feature"][forest["feature"] >= 0].tolist()))
    features = [65, 4, 0, 30] + unused[:1]
    result = model.permutation_importance(rows, target, n_repeats=3, seed=77, features=features)
    counters, gap = oracle.inspect(forest, rows, target, oracle.permutation_jobs(features, 3), 77)
    assert gap >= cases.PROBABILITY_GAP
    expected = oracle.permutation_importance(counters, rows.shape[0], len(features), 3)
    assert result.counters.tobytes() == counters.tobytes()
    assert result.baseline == expected["baseline"] and result.baseline_error == expected["baseline_error"]
    for key in ("error_matrix", "errors", "importance", "importance_std", "margin_shift"):
        assert getattr(result, key).tobytes() == expected[key].tobytes(), key
    assert result.order().tolist() == oracle.importance_order(features, expected["importance"])
    frame = result.frame()
    assert frame["feature"].tolist() == [features[s] for s in result.order()]
    assert (np.diff(frame["importance"].to_numpy()) <= 0).all()
    assert (result.importance != 0).any()
    # by name, all features, other seed and threshold, from HBM
    from doppel_speller_amd import _lib, FEATURE_NAMES
    d_rows, d_target = _lib.DeviceArray.from_host(rows), _lib.DeviceArray.from_host(target)
    everything = model.permutation_importance_device(d_rows, rows.shape[0], d_target, n_repeats=2, seed=78, threshold=0.5)
    counters, gap = oracle.inspect(forest, rows, target, oracle.permutation_jobs(range(66), 2), 78, 0.5)
    assert gap >= cases.PROBABILITY_GAP and everything.counters.tobytes() == counters.tobytes()
    named = model.permutation_importance(rows, target, n_repeats=2, seed=78, threshold=0.5,
                                         features=[FEATURE_NAMES[4], FEATURE_NAMES[65]])
    assert named.features.tolist() == [4, 65] and named.error_matrix.tobytes() == everything.error_matrix[[4, 65]].tobytes()
    if unused:                                       # a feature no tree splits on: the baseline in every repeat
        f = unused[0]
        assert (everything.error_matrix[f] == np.array(everything.baseline)).all()
        assert everything.importance[f] == 0.0 and everything.importance_std[f] == 0.0 and everything.margin_shift[f] == 0.0
    d_rows.free()
    d_target.free()
    model.close()


def test_a_feature_no_tree_splits_on_has_importance_zero():
    case = cases.case("wide_matrix")                 # 10 trees over 96 features: most features are never split on
    forest = case["forest"]
    unused = sorted(set(range(96)) - set(forest["feature"][forest["feature"] >= 0].tolist()))
    assert len(unused) >= 3
    model = model_of(forest, 96)
    result = model.permutation_importance(case["rows"], case["target"], n_repeats=4, seed=3, features=unused[:3])
    assert (result.error_matrix == np.array(result.baseline)).all()
    assert not result.importance.any() and not result.importance_std.any() and not result.margin_shift.any()
    model.close()


def test_partial_dependence_equals_the_oracle():
    import doppel_speller_amd as ds
    case = cases.case("three_row_blocks")
    forest, target = case["forest"], case["target"]
    rows = case["rows"].copy()
    rows[::7, 4] = np.nan
    n = rows.shape[0]
    model = model_of(forest, 66)

    def check(result, feature, grid, target_):
        counters, gap = oracle.inspect(forest, rows, target_, oracle.dependence_jobs(feature, grid), 0)
        assert gap >= cases.PROBABILITY_GAP
        expected = oracle.partial_dependence(counters, n)
        assert result.grid.dtype == np.float32 and result.grid.tobytes() == np.asarray(grid, np.float32).tobytes()
        assert result.counters.tobytes() == counters.tobytes() and result.feature == feature
        assert result.baseline_mean_margin == expected["baseline_mean_margin"]
        assert result.mean_margin.tobytes() == expected["mean_margin"].tobytes()
        assert result.positive_share.tobytes() == expected["positive_share"].tobytes()

    default = model.partial_dependence(rows, 4, n_grid=8)
    grid = oracle.quantile_grid(rows[:, 4], 8)
    assert grid.shape[0] == 9 and np.isnan(grid[-1])
    check(default, 4, grid, None)
    explicit = [np.nan, -5.0, 0.5, 50.0, np.inf]
    check(model.partial_dependence(rows, 7, grid=explicit, target=target), 7, explicit, target)
    by_name = model.partial_dependence(rows, "title_ratio", n_grid=8)
    assert ds.FEATURE_NAMES.index("title_ratio") == 4 and by_name.counters.tobytes() == default.counters.tobytes()
    d_rows = ds._lib.DeviceArray.from_host(rows)
    check(model.partial_dependence_device(d_rows, n, "title_ratio", explicit), 4, explicit, None)
    d_rows.free()
    model.close()


# ---- 4. the partial dependence of a constrained model is monotone -----------------------------------------------------------------
def test_partial_dependence_of_a_monotone_model_is_monotone():
    """y follows a bump of feature 0 and a dip of feature 1, so the free model's partial dependence goes up and down
    along both.  Under +1 on feature 0 and -1 on feature 1 every row's float32 leaf sum is monotone in the feature, and
    so is each row's rounded term and their integer sum: exactly, with no tolerance."""
    import doppel_speller_amd as ds
    rng = np.random.RandomState(5)
    x = rng.uniform(0, 100, (400, 7)).astype(np.float32)
    bump = (x[:, 0] > 30) & (x[:, 0] < 70)
    dip = (x[:, 1] < 25) | (x[:, 1] > 75)
    y = ((bump & dip) ^ (rng.rand(400) < 0.05)).astype(np.float32)
    constraints = np.array([1, -1, 0, 0, 0, 0, 0], np.int8)
    parameters = dict(num_boost_round=20, max_depth=3, eta=0.3)
    bound = ds.ForestTrainer().fit(x, y, monotone_constraints=constraints, **parameters)
    free = ds.ForestTrainer().fit(x, y, **parameters)
    assert bound.monotone_violations(constraints) == 0 and free.monotone_violations(constraints) > 0
    grid = np.linspace(2, 98, 16).astype(np.float32)
    moved = 0
    for feature, sign in ((0, 1), (1, -1)):
        steps = np.diff(bound.partial_dependence(x, feature, grid=grid).mean_margin) * sign
        assert (steps >= 0).all(), (feature, steps)
        moved += int((steps > 0).any())
        steps = np.diff(free.partial_dependence(x, feature, grid=grid).mean_margin)
        assert (steps < 0).any() and (steps > 0).any(), (feature, steps)      # the data is not monotone: no vacuous pass
    assert moved >= 1
    bound.close()
    free.close()


# ---- 5. train_model ----------------------------------------------------------------------------------------------------------------
def test_train_model_permutation_importance():
    import doppel_speller_amd as ds
    from doppel_speller_amd import synth
    w = synth.make_workload(20000, 4000, seed=21, query_seed=22)
    truth, train = synth._to_strings(w.t_flat, w.t_off), synth._to_strings(w.q_flat, w.q_off)
    ids = np.where(w.actual_row >= 0, w.title_id[np.maximum(w.actual_row, 0)], -1)
    fit = dict(num_boost_round=30, early_stopping_rounds=10)
    result = ds.train_model(truth, w.title_id, train, ids, seed=9, transform=False, permutation_repeats=2,
                            permutation_seed=11, **fit)
    got = result.permutation_importance
    assert "permutation" in result.timings and got.n_repeats == 2 and got.seed == 11
    assert got.features.tolist() == list(range(ds.FEATURES_COUNT)) and got.baseline == result.error_matrix
    fe = ds.FeatureEngineering(truth, w.title_id, train, ids, seed=9, transform=False)
    _, _, evaluation, evaluation_target = fe.generate_train_and_evaluation_data_sets()
    expected = result.model.permutation_importance(evaluation, evaluation_target, n_repeats=2, seed=11)
    assert got.n == evaluation.shape[0] and got.counters.tobytes() == expected.counters.tobytes()
    for key in ("error_matrix", "errors", "importance", "importance_std", "margin_shift"):
        assert getattr(got, key).tobytes() == getattr(expected, key).tobytes(), key
    plain = ds.train_model(truth, w.title_id, train, ids, seed=9, transform=False, **fit)
    assert plain.permutation_importance is None and "permutation" not in plain.timings
    assert set(result.timings) - set(plain.timings) == {"permutation"}
    assert all(plain.model.arrays[key].tobytes() == result.model.arrays[key].tobytes()
               for key in ("feature", "threshold", "yes", "no", "missing", "tree_offsets"))
