"""CPU checks of the training-set generation: the restatement (tests/training_set_oracle.py) against what the
reference's own functions produced (tests/golden/make_golden_training.py), the evaluation split, and the checks
FeatureEngineering makes before any device work."""
import os

import numpy as np
import pytest

import training_set_oracle as ts

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _strings(array):
    return [bytes(x).decode("utf-8") for x in array]


@pytest.fixture(scope="module")
def misspell_cases():
    return dict(np.load(os.path.join(GOLDEN, "misspell_cases.npz"), allow_pickle=False))


@pytest.fixture(scope="module")
def training_fixture():
    return dict(np.load(os.path.join(GOLDEN, "training_rows.npz"), allow_pickle=False))


def test_stream_known_answers():
    # splitmix64 of state 0x9e3779b97f4a7c15 (seed 1) after the two discarded outputs; below() is the high product half
    stream = ts.Stream(0, 0, 0)
    first = stream.next()
    again = ts.Stream(0, 0, 0)
    assert again.next() == first
    assert ts.Stream(0, 0, 0).below(1) == 0
    stream = ts.Stream(7, 2, 11)
    x = ts.Stream(7, 2, 11).next()
    assert stream.below(100) == (x * 100) >> 64
    assert ts.Stream(1, 1, 0).next() != ts.Stream(1, 2, 0).next() != ts.Stream(1, 1, 1).next()


def test_sample_is_partial_fisher_yates():
    for seed in range(50):
        pool = list(range(100))
        sample = ts.Stream(seed, 2, 3).sample(pool, 10)
        assert len(set(sample)) == 10 and all(0 <= s < 100 for s in sample)
        assert pool == list(range(100))          # the population is not touched
    assert sorted(ts.Stream(5, 2, 0).sample(range(16), 16)) == list(range(16))


def test_neighbour_table_equals_the_references(misspell_cases):
    letters = "abcdefghijklmnopqrstuvwxyz"
    table = np.zeros((26, 26), dtype=bool)
    for code, near in ts.NEIGHBOURS.items():
        assert near == sorted(near)
        for other in near:
            table[letters.index(ts.ALPHABET[code]), letters.index(ts.ALPHABET[other])] = True
    assert np.array_equal(table, misspell_cases["neighbours"])
    assert ts.ALPHABET.index("n") in ts.NEIGHBOURS[ts.ALPHABET.index("m")]     # same coordinate: kept as a neighbour


def test_oracle_misspellings_equal_the_reference(misspell_cases):
    seed = int(misspell_cases["seed"])
    titles, expected = _strings(misspell_cases["titles"]), _strings(misspell_cases["expected"])
    assert len(titles) >= 2000
    got = [ts.misspell(title, seed, index) for index, title in enumerate(titles)]
    assert got == expected
    assert sum(a != b for a, b in zip(titles, got)) > 0.9 * len(titles)
    assert max(len(t) for t in titles) == 255 and min(len(t) for t in titles) == 3


def test_oracle_rows_equal_the_reference(training_fixture, oracle):
    """_prepare_training_input_data on the fixture's slice: kinds, titles, truth titles and targets, in order, except
    the rows of train titles whose top-100 has a near-tie at the cut."""
    import doppel_speller_amd as ds
    from doppel_speller_amd.match_maker import NativeProblem
    from doppel_speller_amd.training_set import validate_training
    g = training_fixture
    truth = ds.transform_titles(_strings(g["truth_titles"]))
    train = ds.transform_titles(_strings(g["train_titles"]))
    top_n, sample_n, seed = int(g["top_n"]), int(g["sample_n"]), int(g["seed"])
    _, _, train_rows = validate_training(truth, g["truth_ids"], train, g["train_ids"], top_n, sample_n, seed,
                                         {"generated": 0.05})
    problem = NativeProblem(truth, train)
    a = problem.arrays()
    top = oracle.jaccard_topk(a["rowptr"], a["truth_idx"], a["idf32"], a["sums32"], a["q_rowptr"], a["q_cols"],
                              a["q_maxint"], top_n)
    rows = ts.training_rows(truth, train_rows, lambda i: list(top[i]), sample_n, seed)
    assert len(rows) == g["kind"].shape[0]
    kind = np.array([r[0] for r in rows])
    assert np.array_equal(kind, g["kind"])
    query = [train[r[1]] if r[0] != ts.KIND_GENERATED else r[4] for r in rows]
    truth_title = [truth[r[2]] for r in rows]
    target = np.array([r[3] for r in rows])
    near_tie = np.array([r[0] != ts.KIND_GENERATED and bool(g["near_tie"][r[1]]) for r in rows])
    keep = ~near_tie
    assert keep.sum() > 0.95 * len(rows)
    assert [q for q, k in zip(query, keep) if k] == [q for q, k in zip(_strings(g["title"]), keep) if k]
    assert [t for t, k in zip(truth_title, keep) if k] == [t for t, k in zip(_strings(g["truth_title"]), keep) if k]
    assert np.array_equal(target[keep], g["target"][keep])
    assert set(np.unique(g["kind"])) == {1, 2, 3} and (g["train_ids"] == -1).sum() >= 50
    assert np.unique(g["train_ids"][g["train_ids"] >= 0]).shape[0] < (g["train_ids"] >= 0).sum()   # repeated ids


def test_row_plan_matches_the_oracle():
    from doppel_speller_amd.training_set import row_plan
    rng = np.random.RandomState(3)
    for _ in range(20):
        rows = rng.randint(-1, 30, rng.randint(0, 200))
        negative, positive = row_plan(rows)
        expected = ts.row_plan(rows)
        assert negative.tolist() == expected[0] and positive.tolist() == expected[1]


def test_split_sizes_disjoint_deterministic():
    from doppel_speller_amd.training_set import evaluation_split
    rng = np.random.RandomState(0)
    kind = rng.choice([1, 2, 3], 5000, p=[0.4, 0.3, 0.3]).astype(np.uint8)
    train, evaluation = evaluation_split(kind, 7)
    assert np.array_equal(np.sort(np.concatenate((train, evaluation))), np.arange(5000))
    assert np.intersect1d(train, evaluation).shape[0] == 0
    assert (np.diff(train) > 0).all() and (np.diff(evaluation) > 0).all()
    for code, fraction in ((1, 0.05), (2, 0.10), (3, 0.05)):
        assert (kind[evaluation] == code).sum() == int(5000 * fraction)
    again = evaluation_split(kind, 7)
    assert np.array_equal(again[1], evaluation) and np.array_equal(again[0], train)
    assert not np.array_equal(evaluation_split(kind, 8)[1], evaluation)
    assert all(np.array_equal(a, b) for a, b in zip(ts.evaluation_split(kind, 7), (train, evaluation)))
    custom = evaluation_split(kind, 7, {"negative": 0.0, "generated": 0.2})[1]
    assert (kind[custom] == 2).sum() == 0 and (kind[custom] == 1).sum() == 1000


def test_split_raises_when_a_kind_is_short():
    from doppel_speller_amd.training_set import evaluation_split
    kind = np.array([1] * 90 + [2] * 5 + [3] * 5, dtype=np.uint8)      # 10 negative rows wanted, 5 exist
    with pytest.raises(ValueError, match="negative"):
        evaluation_split(kind, 0)
    kind = np.array([2] * 50 + [3] * 50, dtype=np.uint8)
    with pytest.raises(ValueError, match="generated"):
        evaluation_split(kind, 0)


def _no_library(monkeypatch):
    from doppel_speller_amd import _lib

    def refuse():
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "lib", refuse)


@pytest.mark.parametrize("change, message", [
    (dict(truth_title_ids=[1, 2]), "title ids"),
    (dict(truth_title_ids=[1, 1, 2]), "unique"),
    (dict(truth_title_ids=[1.0, 2.0, 3.0]), "integers"),
    (dict(train_title_ids=[1]), "train title ids"),
    (dict(train_title_ids=[1.0, 2.0]), "integers"),
    (dict(train_title_ids=[-2, 1]), "-1"),
    (dict(train_title_ids=[4, 1]), "not truth title ids"),
    (dict(top_n=4), "exceeds"),
    (dict(top_n=0), "top_n"),
    (dict(sample_n=0), "sample_n"),
    (dict(sample_n=17, top_n=3), "sample_n"),
    (dict(sample_n=3, top_n=2), "exceeds top_n"),
    (dict(seed=-1), "seed"),
    (dict(seed=1.5), "seed"),
    (dict(chunk_queries=0), "chunk_queries"),
    (dict(evaluation_fractions={"negative": 1.0}), r"\[0, 1\)"),
    (dict(evaluation_fractions={"positive": -0.1}), r"\[0, 1\)"),
    (dict(evaluation_fractions={"other": 0.1}), "unknown"),
])
def test_validation_errors_without_the_library(monkeypatch, change, message):
    import doppel_speller_amd as ds
    _no_library(monkeypatch)
    arguments = dict(truth_titles=["alpha one", "beta two", "gamma three"], truth_title_ids=[1, 2, 3],
                     train_titles=["alpha", "gama"], train_title_ids=[1, -1], top_n=3, sample_n=2)
    arguments.update(change)
    with pytest.raises(ValueError, match=message):
        ds.FeatureEngineering(**arguments)


def test_valid_arguments_need_no_library(monkeypatch):
    import doppel_speller_amd as ds
    _no_library(monkeypatch)
    fe = ds.FeatureEngineering(["alpha one", "beta two", "gamma three"], [5, 2, 9], ["alpha", "gama", "x"], [9, -1, 9],
                               top_n=3, sample_n=2, seed=3)
    assert fe.train_truth_rows.tolist() == [2, -1, 2]


def test_misspelled_names_checks_without_the_library(monkeypatch):
    import doppel_speller_amd as ds
    _no_library(monkeypatch)
    assert ds.generate_misspelled_names([]) == []
    for bad in (["ab"], ["a" * 256], ["   "]):
        with pytest.raises(ValueError, match="transformed title"):
            ds.generate_misspelled_names(bad)
    with pytest.raises(ValueError, match="seed"):
        ds.generate_misspelled_names(["abc"], seed=-3)
