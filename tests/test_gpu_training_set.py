"""The training set of the match model on the device (ds_misspell_titles, ds_training_pairs_device, FeatureEngineering),
bit-exact against the CPU restatement (tests/training_set_oracle.py) and the vectors captured from the reference
(tests/golden/make_golden_training.py)."""
import ctypes
import os

import numpy as np
import pytest

import training_set_oracle as ts

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _strings(array):
    return [bytes(x).decode("utf-8") for x in array]


def _expected_features(oracle, queries, truth_titles, truth_rows, n_truth):
    """oracle.construct_features of (query title i, truth title truth_rows[i])."""
    import doppel_speller_amd as ds
    from doppel_speller_amd.feature_engineering import truth_word_counts
    from doppel_speller_amd.prediction import _pack
    q_enc, q_len = ds.encode_titles(queries)
    t_enc, t_len = ds.encode_titles(truth_titles)
    chars, offsets = _pack(truth_titles)
    counts = truth_word_counts(chars, offsets, separators=(ord(" "),))
    rows = np.asarray(truth_rows, dtype=np.int64)
    return oracle.construct_features(q_len, t_len[rows], q_enc, t_enc[rows], counts[rows], ds.SPACE_CODE, n_truth)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.fixture(scope="module")
def synthetic():
    """20k truth titles, 4k train titles: 60 % misspelled truth titles (repeated ids among them), 40 % made up (-1)."""
    from doppel_speller_amd import synth
    w = synth.make_workload(20000, 4000, seed=21, query_seed=22)
    truth = synth._to_strings(w.t_flat, w.t_off)
    train = synth._to_strings(w.q_flat, w.q_off)
    ids = np.where(w.actual_row >= 0, w.title_id[np.maximum(w.actual_row, 0)], -1)
    return w, truth, train, ids


def test_misspelling_kernel_equals_the_reference():
    import doppel_speller_amd as ds
    g = dict(np.load(os.path.join(GOLDEN, "misspell_cases.npz"), allow_pickle=False))
    titles = _strings(g["titles"])
    assert ds.generate_misspelled_names(titles, seed=int(g["seed"])) == _strings(g["expected"])


def test_misspelling_kernel_equals_the_oracle_at_scale():
    import doppel_speller_amd as ds
    from doppel_speller_amd import synth
    _, t_flat, t_off = synth.make_truth(200000, seed=5)
    titles = [t for t in synth._to_strings(t_flat, t_off) if len(t) >= 3]    # a few synthetic titles are shorter
    assert len(titles) > 190000
    titles += _strings(np.load(os.path.join(GOLDEN, "misspell_cases.npz"))["titles"])[-40:]
    seed = 123456789012345
    got = ds.generate_misspelled_names(titles, seed=seed)
    expected = [ts.misspell(title, seed, index) for index, title in enumerate(titles)]
    bad = [i for i, (a, b) in enumerate(zip(got, expected)) if a != b]
    assert not bad, [(titles[i], got[i], expected[i]) for i in bad[:5]]
    assert ds.generate_misspelled_names(titles[:1000], seed=seed + 1) != got[:1000]


def test_misspelling_rejects_what_is_not_a_transformed_title():
    import doppel_speller_amd as ds
    from doppel_speller_amd import _lib
    from doppel_speller_amd.training_set import misspell_table
    enc = np.zeros((3, 255), dtype=np.uint8)
    enc[:, :4] = [2, 3, 1, 4]
    lengths = np.array([4, 2, 4], dtype=np.uint8)          # row 1 is too short
    table = ds.TitleTable(enc, lengths, None, 0)
    assert len(misspell_table(table, [0, 2], 0).strings()) == 2
    with pytest.raises(_lib.DoppelError, match="not transformed titles"):
        misspell_table(table, [0, 1], 0)
    with pytest.raises(_lib.DoppelError, match="out of range"):
        misspell_table(table, [0, 3], 0)


@pytest.mark.parametrize("top_n, sample_n", [(top_n, sample_n) for top_n in (10, 17, 100) for sample_n in (1, 10, 16)
                                              if sample_n <= top_n]
                         + [(1, 1), (2, 2), (16, 16), (11, 3)])      # sample_n == top_n: the last step draws below(1)
def test_sampler_equals_the_oracle(top_n, sample_n):
    from doppel_speller_amd import _lib
    rng = np.random.RandomState(top_n * 100 + sample_n)
    n, q_first, n_truth, seed = 3000, 5, 50000, 2 ** 63 + 17
    rows = np.stack([rng.choice(n_truth, top_n, replace=False) for _ in range(n)]).astype(np.int32)
    case = rng.randint(0, 3, n)                             # 0: own row among the candidates, 1: not, 2: no own row
    own = np.where(case == 0, rows[np.arange(n), rng.randint(0, top_n, n)], n_truth + rng.randint(0, 100, n))
    own = np.where(case == 2, -1, own).astype(np.int32)
    index = rng.randint(0, 2 ** 40, n).astype(np.int64)
    total = (q_first + n) * sample_n
    d = {name: _lib.DeviceArray.from_host(array) for name, array in
         (("rows", rows), ("index", index), ("own", own))}
    out = {name: _lib.DeviceArray((total,), dtype) for name, dtype in
           (("q", np.int32), ("t", np.int32), ("y", np.float32))}
    _lib.check(_lib.lib().ds_training_pairs_device(
        d["rows"].ptr, n, top_n, sample_n, d["index"].ptr, d["own"].ptr, ctypes.c_uint64(seed), q_first,
        out["q"].ptr, out["t"].ptr, out["y"].ptr, None), "ds_training_pairs_device")
    pair_q, pair_t, target = (out[k].to_host()[q_first * sample_n:].reshape(n, sample_n) for k in ("q", "t", "y"))
    for i in range(n):
        sample, expected_target = ts.sample_candidates(rows[i].tolist(), sample_n, int(own[i]), seed, int(index[i]))
        assert pair_t[i].tolist() == sample, (i, case[i])
        assert target[i].tolist() == expected_target
        assert (pair_q[i] == q_first + i).all()
    assert (target.sum(axis=1) == (case != 2)).all()       # exactly one own row where there is one


def test_sampler_rejects_bad_arguments():
    from doppel_speller_amd import _lib
    p = _lib.pointer(None)
    for top_n, sample_n in ((10, 0), (10, 11), (100, 17)):
        status = _lib.lib().ds_training_pairs_device(p, 1, top_n, sample_n, p, p, ctypes.c_uint64(0), 0, p, p, p, p)
        assert status == -1


def test_training_rows_equal_the_reference(oracle):
    import doppel_speller_amd as ds
    g = dict(np.load(os.path.join(GOLDEN, "training_rows.npz"), allow_pickle=False))
    fe = ds.FeatureEngineering(_strings(g["truth_titles"]), g["truth_ids"], _strings(g["train_titles"]), g["train_ids"],
                               top_n=int(g["top_n"]), sample_n=int(g["sample_n"]), seed=int(g["seed"]),
                               evaluation_fractions={"negative": 0.05})   # 600 negative rows of 6,974: 10 % is too many
    train, train_target, evaluation, evaluation_target = fe.generate_train_and_evaluation_data_sets()
    rows = fe.rows
    assert rows.shape[0] == g["kind"].shape[0]
    assert np.array_equal(rows["kind"].to_numpy(), g["kind"])
    kind = rows["kind"].to_numpy()
    generated = kind == ts.KIND_GENERATED
    query = np.array(fe.train_titles, dtype=object)[np.where(generated, 0, rows["query_index"].to_numpy())]
    query[generated] = fe.misspelled_titles
    truth_title = np.array(fe.truth_titles, dtype=object)[rows["truth_row"].to_numpy()]
    keep = ~(~generated & g["near_tie"][np.where(generated, 0, rows["query_index"].to_numpy())])
    assert keep.sum() > 0.95 * keep.shape[0]
    assert query[keep].tolist() == np.array(_strings(g["title"]), dtype=object)[keep].tolist()
    assert truth_title[keep].tolist() == np.array(_strings(g["truth_title"]), dtype=object)[keep].tolist()
    assert np.array_equal(rows["target"].to_numpy()[keep], g["target"][keep].astype(np.float32))
    expected = _expected_features(oracle, list(query), fe.truth_titles, rows["truth_row"].to_numpy(),
                                  len(fe.truth_titles))
    assert _same_bits(fe.features, expected)
    evaluation_rows = np.nonzero(rows["evaluation"].to_numpy())[0]
    assert _same_bits(evaluation, expected[evaluation_rows])
    assert _same_bits(train, expected[~rows["evaluation"].to_numpy()])
    assert train.dtype == np.float32 and train_target.dtype == np.float32
    assert np.array_equal(evaluation_target, rows["target"].to_numpy()[evaluation_rows])
    assert set(fe.timings) >= {"top_k", "sample_pairs", "misspell", "features", "split"}


@pytest.fixture(scope="module")
def synthetic_run(synthetic):
    import doppel_speller_amd as ds
    w, truth, train, ids = synthetic
    fe = ds.FeatureEngineering(truth, w.title_id, train, ids, seed=9, transform=False)
    return fe, fe.generate_train_and_evaluation_data_sets()


def test_synthetic_workload_equals_the_oracle(synthetic, synthetic_run, oracle):
    from doppel_speller_amd.match_maker import NativeProblem
    w, truth, train, ids = synthetic
    fe, (train_x, train_y, eval_x, eval_y) = synthetic_run
    problem = NativeProblem(truth, train)
    a = problem.arrays()
    top = oracle.jaccard_topk(a["rowptr"], a["truth_idx"], a["idf32"], a["sums32"], a["q_rowptr"], a["q_cols"],
                              a["q_maxint"], 100)
    assert len(set(ids[ids >= 0].tolist())) < (ids >= 0).sum() and (ids < 0).sum() > 1000
    expected = ts.training_rows(truth, fe.train_truth_rows, lambda i: list(top[i]), 10, 9)
    rows = fe.rows
    assert rows["kind"].tolist() == [r[0] for r in expected]
    assert rows["query_index"].tolist() == [r[1] for r in expected]
    assert rows["truth_row"].tolist() == [r[2] for r in expected]
    assert rows["target"].tolist() == [float(r[3]) for r in expected]
    assert fe.misspelled_titles == [r[4] for r in expected if r[0] == ts.KIND_GENERATED]
    queries = [train[r[1]] if r[0] != ts.KIND_GENERATED else r[4] for r in expected]
    features = _expected_features(oracle, queries, truth, [r[2] for r in expected], len(truth))
    assert _same_bits(fe.features, features)
    kind = rows["kind"].to_numpy()
    train_rows, evaluation_rows = ts.evaluation_split(kind, 9)
    assert _same_bits(train_x, features[train_rows]) and _same_bits(eval_x, features[evaluation_rows])
    target = rows["target"].to_numpy()
    assert np.array_equal(train_y, target[train_rows]) and np.array_equal(eval_y, target[evaluation_rows])


def test_synthetic_chunking_repeats_and_seeds(synthetic, synthetic_run):
    import doppel_speller_amd as ds
    w, truth, train, ids = synthetic
    fe, first = synthetic_run
    again = fe.generate_train_and_evaluation_data_sets()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))
    chunked = ds.FeatureEngineering(truth, w.title_id, train, ids, seed=9, transform=False, chunk_queries=7)
    result = chunked.generate_train_and_evaluation_data_sets()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, result))
    assert chunked.rows.equals(fe.rows) and chunked.misspelled_titles == fe.misspelled_titles
    other = ds.FeatureEngineering(truth, w.title_id, train, ids, seed=10, transform=False)
    other.generate_train_and_evaluation_data_sets()
    differ = sum(a != b for a, b in zip(other.misspelled_titles, fe.misspelled_titles))
    assert differ > 0.5 * len(fe.misspelled_titles)


def test_trained_model_beats_the_random_ensemble(synthetic, synthetic_run):
    """ForestTrainer.fit on the generated set, then Prediction on held-out queries (another query seed)."""
    import doppel_speller_amd as ds
    from doppel_speller_amd import synth
    w, truth, _, _ = synthetic
    fe, (train_x, train_y, eval_x, eval_y) = synthetic_run
    model = ds.ForestTrainer().fit(train_x, train_y, eval_x, eval_y)
    held_out = synth.make_workload(20000, 2000, seed=21, query_seed=23)
    queries = synth._to_strings(held_out.q_flat, held_out.q_off)
    expected = np.where(held_out.actual_row >= 0, w.title_id[np.maximum(held_out.actual_row, 0)], -1)

    def accuracy(forest):
        answer = ds.Prediction(truth, w.title_id, forest, transform=False).generate_test_predictions(queries)
        return float(np.mean(answer["title_id"].to_numpy() == expected))

    stand_in = synth.make_forest(n_trees=100)
    random_model = ds.ForestModel(stand_in["feature"], stand_in["threshold"], stand_in["yes"], stand_in["no"],
                                  stand_in["missing"], stand_in["tree_offsets"], stand_in["n_features"],
                                  stand_in["base_margin"])
    trained, random_ = accuracy(model), accuracy(random_model)
    print(f"held-out accuracy: trained {trained:.4f}, random ensemble {random_:.4f}, {model.n_trees} trees")
    assert trained > random_
