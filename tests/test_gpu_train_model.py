"""train_model and FeatureEngineering.generate_device_data_sets on the 20k x 4k synthetic workload at seed 9, against
the host chain that exists without them: generate_train_and_evaluation_data_sets -> ForestTrainer.fit ->
feature_importance / evaluation_error_matrix.  Everything is compared bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
MODEL_KEYS = ("feature", "threshold", "yes", "no", "missing", "tree_offsets")
FIT = dict(num_boost_round=120, early_stopping_rounds=20)


@pytest.fixture(scope="module")
def synthetic():
    """20k truth titles, 4k train titles: 60 % misspelled truth titles (repeated ids among them), 40 % made up (-1)."""
    from doppel_speller_amd import synth
    w = synth.make_workload(20000, 4000, seed=21, query_seed=22)
    truth = synth._to_strings(w.t_flat, w.t_off)
    train = synth._to_strings(w.q_flat, w.q_off)
    ids = np.where(w.actual_row >= 0, w.title_id[np.maximum(w.actual_row, 0)], -1)
    return w, truth, train, ids


@pytest.fixture(scope="module")
def host_chain(synthetic):
    import doppel_speller_amd as ds
    w, truth, train, ids = synthetic
    fe = ds.FeatureEngineering(truth, w.title_id, train, ids, seed=9, transform=False)
    sets = fe.generate_train_and_evaluation_data_sets()
    trainer = ds.ForestTrainer()
    model = trainer.fit(*sets, **FIT)
    return fe, sets, trainer, model


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_device_data_sets_equal_the_host_sets(synthetic, host_chain):
    import doppel_speller_amd as ds
    w, truth, train, ids = synthetic
    host_fe, host_sets, _, _ = host_chain
    fe = ds.FeatureEngineering(truth, w.title_id, train, ids, seed=9, transform=False)
    sets = fe.generate_device_data_sets()
    assert fe.features is None and fe.misspelled_titles is None and sets.features is None
    for got, want in zip(sets.to_host(), host_sets):
        assert same_bits(got, want)
    assert sets.n_train == host_sets[0].shape[0] and sets.n_evaluation == host_sets[2].shape[0] > 0
    assert fe.rows.equals(host_fe.rows)
    assert sets.misspelled_titles() == host_fe.misspelled_titles
    assert "gather" in fe.timings and set(fe.timings) >= set(host_fe.timings)

    chunked = ds.FeatureEngineering(truth, w.title_id, train, ids, seed=9, transform=False, chunk_queries=7)
    chunked_sets = chunked.generate_device_data_sets(keep_features=True)
    for got, want in zip(chunked_sets.to_host(), host_sets):
        assert same_bits(got, want)
    assert chunked.rows.equals(host_fe.rows) and chunked_sets.misspelled_titles() == host_fe.misspelled_titles
    assert same_bits(chunked_sets.features.to_host(chunked_sets.n_rows), host_fe.features)
    again = fe.generate_device_data_sets()                               # the same object, a second call
    for got, want in zip(again.to_host(), host_sets):
        assert same_bits(got, want)


def test_train_model_equals_the_host_chain(synthetic, host_chain):
    import doppel_speller_amd as ds
    from doppel_speller_amd import synth
    w, truth, train, ids = synthetic
    host_fe, (train_x, train_y, eval_x, eval_y), host_trainer, host_model = host_chain
    result = ds.train_model(truth, w.title_id, train, ids, seed=9, transform=False, **FIT)
    assert isinstance(result, ds.TrainModelResult)
    for key in MODEL_KEYS:
        assert same_bits(result.model.arrays[key], host_model.arrays[key]), key
    assert result.model.arrays["base_margin"] == host_model.arrays["base_margin"]
    assert result.best_iteration == host_trainer.best_iteration and result.history == host_trainer.history
    assert result.model.n_trees == result.best_iteration + 1 > 1
    assert same_bits(result.feature_importance, host_model.feature_importance())
    assert result.error_matrix == ds.evaluation_error_matrix(host_model, eval_x, eval_y)
    assert sum(result.error_matrix) == eval_y.shape[0]
    assert result.rows.equals(host_fe.rows)
    assert {"features", "gather", "cuts", "bin", "boost", "evaluate", "total"} <= set(result.timings)
    assert result.timings["total"] >= result.timings["boost"] > 0

    second = ds.train_model(truth, w.title_id, train, ids, seed=9, transform=False, **FIT)
    for key in MODEL_KEYS:
        assert second.model.arrays[key].tobytes() == result.model.arrays[key].tobytes(), key
    assert second.error_matrix == result.error_matrix and second.history == result.history
    assert second.feature_importance.tobytes() == result.feature_importance.tobytes()

    held_out = synth.make_workload(20000, 2000, seed=21, query_seed=23)
    queries = synth._to_strings(held_out.q_flat, held_out.q_off)
    expected = np.where(held_out.actual_row >= 0, w.title_id[np.maximum(held_out.actual_row, 0)], -1)

    def accuracy(forest):
        answer = ds.Prediction(truth, w.title_id, forest, transform=False).generate_test_predictions(queries)
        return float(np.mean(answer["title_id"].to_numpy() == expected))

    one_call, chain = accuracy(result.model), accuracy(host_model)
    print(f"held-out accuracy: train_model {one_call:.4f}, host chain {chain:.4f}, {result.model.n_trees} trees")
    assert one_call == chain


def test_train_model_without_an_evaluation_set(synthetic):
    import doppel_speller_amd as ds
    w, truth, train, ids = synthetic
    none = {"generated": 0, "negative": 0, "positive": 0}
    result = ds.train_model(truth, w.title_id, train, ids, seed=9, transform=False, evaluation_fractions=none,
                            num_boost_round=8)
    fe = ds.FeatureEngineering(truth, w.title_id, train, ids, seed=9, transform=False, evaluation_fractions=none)
    train_x, train_y, eval_x, eval_y = fe.generate_train_and_evaluation_data_sets()
    assert eval_x.shape[0] == 0
    host_model = ds.ForestTrainer().fit(train_x, train_y, num_boost_round=8)
    assert result.error_matrix is None and result.best_iteration == 7 and result.history == [None] * 8
    for key in MODEL_KEYS:
        assert same_bits(result.model.arrays[key], host_model.arrays[key]), key
