"""Prediction.explain and train_model(cover=True) on the GPU: the explained pair against the candidates ranked_matches
keeps, the contributions against ForestModel.predict_contributions on the explained feature rows (bit for bit), the stage
and answer against generate_test_predictions, and the variants that must not change anything."""
import numpy as np
import pytest

import contributions_cases as cc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def problem():
    """2,000 truth titles, 300 queries (30 of them verbatim truth titles), 40 random trees with a counted cover + 1."""
    import doppel_speller_amd as ds
    from doppel_speller_amd import synth
    w = synth.make_workload(2000, 300, seed=31)
    truth = synth._to_strings(w.t_flat, w.t_off)
    queries = synth._to_strings(w.q_flat, w.q_off)
    rng = np.random.RandomState(32)
    for q, t in zip(rng.permutation(300)[:30], rng.randint(0, 2000, 30)):
        queries[q] = truth[t]
    forest = synth.make_forest(seed=33, n_trees=40)
    model = ds.ForestModel(forest["feature"], forest["threshold"], forest["yes"], forest["no"], forest["missing"],
                           forest["tree_offsets"], forest["n_features"], forest["base_margin"])
    model.fit_cover(cc.random_rows(34, 4000), prior=1.0)
    return truth, np.asarray(w.title_id, dtype=np.int64), queries, model, forest


def _explain(problem, approximate=False, **options):
    import doppel_speller_amd as ds
    truth, ids, queries, model, _ = problem
    p = ds.Prediction(truth, ids, model, top_n=10, transform=False, **options)
    frame = p.explain(queries, approximate=approximate)
    return p, frame


@pytest.fixture(scope="module")
def explained(problem):
    return _explain(problem, chunk_queries=128)


def _same_frame(a, b):
    return list(a.columns) == list(b.columns) and a.dtypes.tolist() == b.dtypes.tolist() and all(
        np.array_equal(np.ascontiguousarray(a[c].to_numpy()).view(np.uint8),
                       np.ascontiguousarray(b[c].to_numpy()).view(np.uint8)) for c in a.columns)


def test_the_explained_pair_is_the_best_candidate(problem, explained):
    import doppel_speller_amd as ds
    truth, ids, queries, model, _ = problem
    p, frame = explained
    assert tuple(frame.columns) == ds.EXPLAIN_COLUMNS and len(frame) == 300
    assert np.array_equal(frame["test_index"].to_numpy(), np.arange(300))
    assert p.details is None and p.candidates is None and p.timings["contributions"] > 0
    other = ds.Prediction(truth, ids, model, top_n=10, transform=False, chunk_queries=128)
    other.ranked_matches(queries, n=1, keep_candidates=True)
    c = other.candidates
    # np.argmax takes a NaN for the maximum, ds_best_pairs_device never lets one replace a candidate: the shortcut below
    # holds only while no probability is a NaN (tests/test_gpu_query_kernels.py compares the kernel with its own loop)
    assert not np.isnan(c.probabilities).any()
    where = np.argmax(c.probabilities, axis=1)                       # the first of the maxima
    assert np.array_equal(frame["match_row"].to_numpy(), c.rows[np.arange(300), where].astype(np.int64))
    assert frame["probability"].dtype == np.float32
    assert np.array_equal(frame["probability"].to_numpy().view(np.uint32),
                          c.probabilities[np.arange(300), where].view(np.uint32))
    assert np.array_equal(frame["title_id"].to_numpy(), ids[frame["match_row"].to_numpy()])


def test_contributions_are_those_of_the_explained_feature_rows(problem, explained):
    truth, ids, queries, model, forest = problem
    p, frame = explained
    assert p.explained_features.shape == (300, 66) and p.explained_features.dtype == np.float32
    assert p.contributions.shape == (300, 66) and p.contributions.dtype == np.float64
    direct = model.predict_contributions(p.explained_features)
    assert np.array_equal(p.contributions.view(np.uint64), direct[:, :66].view(np.uint64))
    assert np.array_equal(frame["bias"].to_numpy().view(np.uint64), direct[:, 66].view(np.uint64))
    margins = model.predict(p.explained_features, output_margin=True)
    assert np.array_equal(frame["margin"].to_numpy().view(np.uint32), margins.view(np.uint32))
    probabilities = model.predict(p.explained_features)
    assert np.array_equal(frame["probability"].to_numpy().view(np.uint32), probabilities.view(np.uint32))
    # local accuracy against the float32 margin, and the device result against the yardstick
    bound = 40 * 2.0 ** -24 * cc.leaf_sum_bound(forest)
    total = p.contributions.sum(axis=1) + frame["bias"].to_numpy()
    assert np.abs(total - frame["margin"].to_numpy().astype(np.float64)).max() <= bound
    expected = cc.tree_shap(forest, model.cover, p.explained_features)
    assert np.abs(direct - expected).max() <= cc.TOL_FACTOR * cc.forest_scale(forest)


def test_stage_and_answer_are_those_of_generate_test_predictions(problem, explained):
    import doppel_speller_amd as ds
    truth, ids, queries, model, _ = problem
    _, frame = explained
    other = ds.Prediction(truth, ids, model, top_n=10, transform=False, chunk_queries=128)
    other.generate_test_predictions(queries)
    details = other.details
    assert np.array_equal(frame["stage"].to_numpy(), details["stage"].to_numpy())
    assert np.array_equal(frame["answer_row"].to_numpy(), details["match_row"].to_numpy())
    assert set(frame["stage"].tolist()) >= {ds.prediction.STAGE_EXACT, ds.prediction.STAGE_NONE}


@pytest.mark.parametrize("options", [dict(chunk_queries=None), dict(chunk_queries=128, prepare_queries="host"),
                                     dict(chunk_queries=7)])
def test_chunking_and_query_preparation_change_nothing(problem, explained, options):
    p, frame = explained
    other, other_frame = _explain(problem, **options)
    assert _same_frame(frame, other_frame)
    assert np.array_equal(p.contributions.view(np.uint64), other.contributions.view(np.uint64))
    assert np.array_equal(p.explained_features.view(np.uint32), other.explained_features.view(np.uint32))


def test_approximate_and_a_shuffled_test_index(problem, explained):
    truth, ids, queries, model, _ = problem
    p, frame = explained
    other, other_frame = _explain(problem, approximate=True, chunk_queries=128)
    direct = model.predict_contributions(other.explained_features, approximate=True)
    assert np.array_equal(other.contributions.view(np.uint64), direct[:, :66].view(np.uint64))
    assert np.array_equal(other_frame["bias"].to_numpy().view(np.uint64), direct[:, 66].view(np.uint64))
    assert np.array_equal(other.explained_features.view(np.uint32), p.explained_features.view(np.uint32))
    assert not np.array_equal(other.contributions, p.contributions)
    for column in ("match_row", "probability", "margin", "stage", "answer_row"):
        assert np.array_equal(other_frame[column].to_numpy(), frame[column].to_numpy())
    index = np.random.RandomState(1).permutation(300) + 1000
    import doppel_speller_amd as ds
    again = ds.Prediction(truth, ids, model, top_n=10, transform=False, chunk_queries=128)
    shuffled = again.explain(queries, test_index=index)
    assert np.array_equal(shuffled["test_index"].to_numpy(), index)          # a line per title, in the titles' order
    assert np.array_equal(shuffled["match_row"].to_numpy(), frame["match_row"].to_numpy())
    assert np.array_equal(again.contributions.view(np.uint64), p.contributions.view(np.uint64))
    assert len(again.explain([])) == 0 and again.contributions.shape == (0, 66)


def test_train_model_with_cover():
    """At the smallest shape of test_gpu_train_model.py (no evaluation set, 8 rounds): the cover is the count of the
    training matrix, the trees are those of cover=False."""
    import doppel_speller_amd as ds
    from doppel_speller_amd import synth
    w = synth.make_workload(20000, 4000, seed=21, query_seed=22)
    truth = synth._to_strings(w.t_flat, w.t_off)
    train = synth._to_strings(w.q_flat, w.q_off)
    ids = np.where(w.actual_row >= 0, w.title_id[np.maximum(w.actual_row, 0)], -1)
    none = {"generated": 0, "negative": 0, "positive": 0}
    arguments = dict(seed=9, transform=False, evaluation_fractions=none, num_boost_round=8)
    plain = ds.train_model(truth, w.title_id, train, ids, **arguments)
    covered = ds.train_model(truth, w.title_id, train, ids, cover=True, **arguments)
    assert plain.model.cover is None and "cover" not in plain.timings and covered.timings["cover"] > 0
    assert set(covered.timings) == set(plain.timings) | {"cover"}
    for key in ("feature", "threshold", "yes", "no", "missing", "tree_offsets"):
        assert covered.model.arrays[key].tobytes() == plain.model.arrays[key].tobytes(), key
    assert covered.history == plain.history and covered.best_iteration == plain.best_iteration
    fe = ds.FeatureEngineering(truth, w.title_id, train, ids, seed=9, transform=False, evaluation_fractions=none)
    train_x = fe.generate_train_and_evaluation_data_sets()[0]
    counts = cc.node_counts(covered.model.arrays, train_x)
    assert covered.model.cover.dtype == np.float64 and np.array_equal(covered.model.cover, counts.astype(np.float64))
    assert np.array_equal(covered.model.read_cover(), covered.model.cover)
    contributions = covered.model.predict_contributions(train_x[:64])
    margins = covered.model.predict(train_x[:64], output_margin=True).astype(np.float64)
    assert np.abs(contributions.sum(axis=1) - margins).max() <= 8 * 2.0 ** -24 * cc.leaf_sum_bound(covered.model.arrays)
