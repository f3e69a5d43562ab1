"""FeatureEngineering.generate_hard_negatives / generate_device_hard_negatives and DeviceDataSets.with_hard_negatives against
an oracle made of pieces that existed before them: the top-k rows of TruthIndex, construct_features_indexed, ForestModel.
predict(output_margin=True), the base set's `rows` for the exclusion, and the NumPy rule of tests/hard_cases.py.  Bit for
bit, for the host and the device form, chunked and not, with the exclusion on and off."""
import numpy as np
import pytest

import hard_cases as hc
from test_forest_cpu import random_dump

pytestmark = pytest.mark.gpu

N_TRUTH, N_TRAIN, WORKLOAD_SEED = 300, 60, 31
TOP_N, SAMPLE_N, HARD_N, BASE_SEED, MODEL_SEED = 20, 4, 3, 9, 6


@pytest.fixture(scope="module")
def workload():
    """300 truth titles, 60 train titles: 60 % misspelled truth titles (repeated ids among them), 40 % made up (-1)."""
    from doppel_speller_amd import synth
    w = synth.make_workload(N_TRUTH, N_TRAIN, seed=WORKLOAD_SEED, query_seed=WORKLOAD_SEED + 1)
    truth = synth._to_strings(w.t_flat, w.t_off)
    train = synth._to_strings(w.q_flat, w.q_off)
    ids = np.where(w.actual_row >= 0, w.title_id[np.maximum(w.actual_row, 0)], -1)
    assert (ids < 0).sum() >= 10 and (ids >= 0).sum() >= 20
    return w.title_id, truth, train, ids


@pytest.fixture(scope="module")
def model():
    """A small fixed forest, not a trained one; base_score 0.5, so training can continue from it."""
    import doppel_speller_amd as ds
    return ds.ForestModel.from_xgboost_dump(random_dump(MODEL_SEED, n_trees=12), ds.FEATURES_COUNT)


def _engineering(workload, chunk_queries=None):
    import doppel_speller_amd as ds
    title_id, truth, train, ids = workload
    return ds.FeatureEngineering(truth, title_id, train, ids, top_n=TOP_N, sample_n=SAMPLE_N, seed=BASE_SEED,
                                 transform=False, chunk_queries=chunk_queries)


@pytest.fixture(scope="module")
def engineered(workload):
    """{chunk_queries: an object with its base set generated}; the base set does not depend on the chunk."""
    out = {}
    for chunk in (None, 7):
        out[chunk] = _engineering(workload, chunk)
        out[chunk].generate_train_and_evaluation_data_sets()
    assert out[7].rows.equals(out[None].rows)
    return out


@pytest.fixture(scope="module")
def scored(workload, engineered, model):
    """The oracle's inputs, computed once: the selected train rows, their candidates' rows and margins, their own rows,
    the rows the base set drew for them, and the two title tables."""
    import doppel_speller_amd as ds
    from doppel_speller_amd.prediction import TruthSide, _pack
    from doppel_speller_amd.training_set import row_plan
    _, truth, train, _ = workload
    fe = engineered[None]
    selected = np.concatenate(row_plan(fe.train_truth_rows))
    titles = [train[i] for i in selected]
    side = TruthSide(truth)
    rows = side.index.top_k(*side.query_rows(*_pack(titles)), TOP_N)
    queries = ds.TitleTable(*ds.encode_titles(titles), None)
    n = selected.shape[0]
    features = ds.construct_features_indexed(queries, side.table, np.repeat(np.arange(n), TOP_N), rows.reshape(-1),
                                             ds.SPACE_CODE, len(truth))
    margins = model.predict(features, output_margin=True).reshape(n, TOP_N)
    base = fe.rows.iloc[:n * SAMPLE_N]
    assert np.array_equal(base["query_index"].to_numpy(), np.repeat(selected, SAMPLE_N))
    sampled = base["truth_row"].to_numpy().reshape(n, SAMPLE_N).astype(np.int32)
    return dict(selected=selected, rows=rows, margins=margins, own=fe.train_truth_rows[selected].astype(np.int32),
                sampled=sampled, queries=queries, side=side, n_truth=len(truth))


def _expected(scored, exclude_sampled, min_margin=None, hard_n=HARD_N):
    """(hard_rows' columns, features) by the NumPy rule."""
    import doppel_speller_amd as ds
    threshold = hc.NO_THRESHOLD if min_margin is None else np.float32(min_margin)
    pair_q, pair_t, position, margin, total = hc.mine_keys(
        scored["rows"], scored["margins"], scored["own"], scored["sampled"] if exclude_sampled else None, scored["n_truth"],
        hard_n, threshold)
    features = ds.construct_features_indexed(scored["queries"], scored["side"].table, pair_q, pair_t, ds.SPACE_CODE,
                                             scored["n_truth"])
    with np.errstate(over="ignore"):
        probability = (np.float32(1.0) / (np.float32(1.0) + np.exp(-margin))).astype(np.float32)
    columns = dict(query_index=scored["selected"][pair_q].astype(np.int64), truth_row=pair_t.astype(np.int64),
                   position=position, margin=margin, probability=probability)
    return columns, features, pair_q


def _same_rows(frame, columns):
    assert tuple(frame.columns) == tuple(columns)
    for name, expected in columns.items():
        got = frame[name].to_numpy()
        assert got.dtype == expected.dtype and got.tobytes() == expected.tobytes(), name


def _mine(fe, model, form, **arguments):
    """(features, target) of either form, the device form read back."""
    import doppel_speller_amd as ds
    if form == "host":
        return fe.generate_hard_negatives(model, **arguments)
    hard = fe.generate_device_hard_negatives(model, **arguments)
    assert isinstance(hard, ds.DeviceHardNegatives) and hard.features.shape == (max(hard.n, 1), ds.FEATURES_COUNT)
    out = hard.to_host()
    hard.free()
    return out


@pytest.mark.parametrize("exclude_sampled", [True, False], ids=["exclude", "keep"])
@pytest.mark.parametrize("chunk", [7, None], ids=["chunks_of_7", "one_chunk"])
@pytest.mark.parametrize("form", ["host", "device"])
def test_mined_rows_equal_the_oracle(engineered, scored, model, form, chunk, exclude_sampled):
    fe = engineered[chunk]
    rows_before, timings_before, features_before = fe.rows.copy(), dict(fe.timings), fe.features
    features, target = _mine(fe, model, form, hard_n=HARD_N, exclude_sampled=exclude_sampled)
    columns, expected, _ = _expected(scored, exclude_sampled)
    _same_rows(fe.hard_rows, columns)
    assert features.dtype == np.float32 and features.shape == expected.shape
    assert features.view(np.uint32).tobytes() == expected.view(np.uint32).tobytes()
    assert target.dtype == np.float32 and target.shape == (expected.shape[0],) and not target.any()
    assert set(fe.hard_timings) == {"top_k", "features", "model", "select", "mined_features", "copy_back"}
    assert all(value >= 0 for value in fe.hard_timings.values()) and fe.hard_timings["select"] > 0
    assert fe.rows.equals(rows_before) and fe.timings == timings_before and fe.features is features_before


def test_the_case_keeps_its_teeth(scored):
    """On the oracle's own values: the threshold cuts a title short, the exclusion takes a candidate that would have been
    mined, and a title fills all its slots."""
    median = np.float32(np.median(scored["margins"]))
    _, _, free_q = _expected(scored, False)
    _, _, held_q = _expected(scored, True)
    _, _, cut_q = _expected(scored, True, min_margin=median)
    n = scored["selected"].shape[0]
    count = lambda pair_q: np.bincount(pair_q, minlength=n)
    assert (count(cut_q) < count(held_q)).any()                          # cut short by the threshold
    assert (count(cut_q) == HARD_N).any()                                # all slots filled, even so
    free, held = _expected(scored, False)[0], _expected(scored, True)[0]
    lost = set(zip(free["query_index"].tolist(), free["truth_row"].tolist())) - \
        set(zip(held["query_index"].tolist(), held["truth_row"].tolist()))
    assert lost                                                          # a candidate lost to the exclusion
    assert (count(free_q) == HARD_N).all() and (scored["own"] >= 0).any() and (scored["own"] < 0).any()


def test_no_mined_pair_is_in_the_base_set_or_the_titles_own(engineered, scored, model):
    fe = engineered[None]
    fe.generate_hard_negatives(model, hard_n=HARD_N)
    mined = set(zip(fe.hard_rows["query_index"].tolist(), fe.hard_rows["truth_row"].tolist()))
    base = fe.rows[fe.rows["kind"] != 1]
    assert len(mined) == len(fe.hard_rows) > 0
    assert not mined & set(zip(base["query_index"].tolist(), base["truth_row"].tolist()))
    own = fe.train_truth_rows[fe.hard_rows["query_index"].to_numpy()]
    assert (own != fe.hard_rows["truth_row"].to_numpy()).all()
    fe.generate_hard_negatives(model, hard_n=HARD_N, exclude_sampled=False)
    kept = set(zip(fe.hard_rows["query_index"].tolist(), fe.hard_rows["truth_row"].tolist()))
    assert kept & set(zip(base["query_index"].tolist(), base["truth_row"].tolist()))     # the exclusion is what did it
    own = fe.train_truth_rows[fe.hard_rows["query_index"].to_numpy()]
    assert (own != fe.hard_rows["truth_row"].to_numpy()).all()


@pytest.mark.parametrize("form", ["host", "device"])
def test_min_margin(engineered, scored, model, form):
    median = float(np.float32(np.median(scored["margins"])))            # from the oracle, not from the code under test
    for chunk in (7, None):
        fe = engineered[chunk]
        features, target = _mine(fe, model, form, hard_n=HARD_N, min_margin=median)
        columns, expected, _ = _expected(scored, True, min_margin=median)
        _same_rows(fe.hard_rows, columns)
        assert features.view(np.uint32).tobytes() == expected.view(np.uint32).tobytes() and target.shape == (len(expected),)
        assert 0 < len(expected) and (fe.hard_rows["margin"].to_numpy() > np.float32(median)).all()
        above = float(scored["margins"].max()) + 1.0
        features, target = _mine(fe, model, form, hard_n=HARD_N, min_margin=above)
        assert features.shape == (0, 66) and features.dtype == np.float32
        assert target.shape == (0,) and target.dtype == np.float32 and len(fe.hard_rows) == 0
        assert tuple(fe.hard_rows.columns) == ("query_index", "truth_row", "position", "margin", "probability")


def test_without_a_base_set_only_the_unexcluded_form_runs(workload, scored, model):
    fe = _engineering(workload)
    with pytest.raises(ValueError, match="generate the base set"):
        fe.generate_hard_negatives(model, hard_n=HARD_N)
    features, _ = fe.generate_hard_negatives(model, hard_n=HARD_N, exclude_sampled=False)
    columns, expected, _ = _expected(scored, False)
    _same_rows(fe.hard_rows, columns)
    assert features.view(np.uint32).tobytes() == expected.view(np.uint32).tobytes() and fe.rows is None


def test_with_hard_negatives_extends_the_training_matrix_in_hbm(workload, scored, model):
    import doppel_speller_amd as ds
    fe = _engineering(workload)
    sets = fe.generate_device_data_sets()
    hard = fe.generate_device_hard_negatives(model, hard_n=HARD_N)
    columns, expected, _ = _expected(scored, True)
    assert hard.n == expected.shape[0] > 0
    before = sets.to_host()
    joined = sets.with_hard_negatives(hard)
    assert joined.n_train == sets.n_train + hard.n and joined.n_evaluation == sets.n_evaluation
    assert joined.n_rows == sets.n_rows + hard.n
    train, train_target, evaluation, evaluation_target = joined.to_host()
    assert train[:sets.n_train].tobytes() == before[0].tobytes()
    assert train[sets.n_train:].view(np.uint32).tobytes() == expected.view(np.uint32).tobytes()
    assert train_target.dtype == np.float32 and train_target[:sets.n_train].tobytes() == before[1].tobytes()
    assert not train_target[sets.n_train:].any() and train_target.shape == (joined.n_train,)
    assert evaluation.tobytes() == before[2].tobytes() and evaluation_target.tobytes() == before[3].tobytes()
    after = sets.to_host()                                               # the old sets are whole, and stay so
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
    hard.free()
    sets.free()
    continued = ds.ForestTrainer().fit_device(joined.train, joined.n_train, joined.train_target, joined.evaluation,
                                              joined.n_evaluation, joined.evaluation_target, init_model=model,
                                              num_boost_round=2)
    assert continued.n_trees in (model.n_trees + 1, model.n_trees + 2)   # the best of the two new rounds
    head = ds.ForestModel.head_arrays(continued.arrays, model.n_trees)
    assert all(head[key].tobytes() == model.arrays[key].tobytes() for key in ds.ForestModel.TREE_KEYS)
    joined.free()
