"""CPU checks of the training-set generation: the restatement (tests/training_set_oracle.py) against what the
reference's own functions produced (tests/golden/make_golden_training.py), the evaluation split, and the checks
FeatureEngineering makes before any device work."""
import os
import re

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


# ---- the misspelling matrix: many draws per edge title, with the edit functions the reference applied ---------------
EDITS = ("swap_word", "add_letter", "remove_letter", "replace_letter", "add_space", "remove_space")
TITLE_CLASSES = {
    "long": lambda t: len(t) >= 253,
    "short": lambda t: len(t) <= 4,
    "digits": lambda t: all(ch in " 0123456789" for ch in t),
    "one word": lambda t: " " not in t,
}
# (class, edit, changed) cells that no title of the class can reach, each with its reason; every other cell of the
# 4 x 6 x 2 table must occur MIN_PER_CELL times among the recorded cases
NEVER = "cannot happen"
UNLIKELY = "needs 11 draws in a row on a space"
IMPOSSIBLE_CELLS = {
    # no edit makes a letter out of a digit or a space, and both functions only accept a letter (:107, :121)
    ("digits", "add_letter", True): NEVER,
    ("digits", "replace_letter", True): NEVER,
    # a one-word title gains a space only through add_space, and only one of add_space / remove_space is drawn (:168)
    ("one word", "remove_space", True): NEVER,
    # remove_letter returns its input only after 11 draws that all land on a space (:94-97).  A transformed title has
    # single spaces between words and no edit puts two spaces side by side before remove_letter runs (add_space
    # refuses a place next to a space, :133), so fewer than half of the characters are spaces: less than 2^-11 per
    # call for any title, and for a one-word title (no space, or one after add_space among >= 3 characters) < 3^-11
    ("long", "remove_letter", False): UNLIKELY,
    ("short", "remove_letter", False): UNLIKELY,
    ("digits", "remove_letter", False): UNLIKELY,
    ("one word", "remove_letter", False): UNLIKELY,
}
MIN_PER_CELL = 3


@pytest.fixture(scope="module")
def matrix():
    g = dict(np.load(os.path.join(GOLDEN, "misspell_matrix.npz"), allow_pickle=False))
    g["titles"], g["expected"], g["edited"] = _strings(g["titles"]), _strings(g["expected"]), _strings(g["edited"])
    g["functions"] = [f.split(",") for f in _strings(g["functions"])]
    return g


def _collapsed(text):
    """Runs of spaces as one, stripped: transform_title (common.py:30) before the cut, for [a-z0-9 ] text."""
    return re.sub(" +", " ", text).strip()


def test_matrix_layout(matrix):
    titles, repeats = matrix["titles"], int(matrix["repeats"])
    assert repeats >= 64 and len(titles) % repeats == 0 and len(titles) >= 3000
    assert all(len(set(titles[i:i + repeats])) == 1 for i in range(0, len(titles), repeats))
    assert len(set(titles)) == len(titles) // repeats
    assert matrix["unchanged"].shape == (len(titles), 2)
    for functions, unchanged in zip(matrix["functions"], matrix["unchanged"]):
        assert 1 <= len(functions) <= 2 and set(functions) <= set(EDITS) and len(set(functions)) == len(functions)
        assert len(functions) == 2 or not unchanged[1]
    for required in ("1" * 255, "1 " * 127 + "1", "k" * 253 + " k", "k" * 252 + " kk", "ab 1", "0 0", "a 1"):
        assert required in titles
    assert any(len(t) == 255 and all(len(w) == 1 for w in t.split(" ")) for t in titles)
    assert any(len(t) == 254 and t[-1].isdigit() for t in titles)


def test_oracle_equals_the_reference_on_the_matrix(matrix):
    seed = int(matrix["seed"])
    got = [ts.misspell(title, seed, index) for index, title in enumerate(matrix["titles"])]
    bad = [i for i, (a, b) in enumerate(zip(got, matrix["expected"])) if a != b]
    assert not bad, [(i, matrix["titles"][i], matrix["functions"][i], got[i], matrix["expected"][i]) for i in bad[:5]]


def test_matrix_covers_every_possible_cell(matrix):
    """Every (title class, edit, changed / returned unchanged) cell that a title of the class can reach occurs at least
    MIN_PER_CELL times in what the reference recorded; the others are listed in IMPOSSIBLE_CELLS with their reason."""
    count = {(name, edit, changed): 0 for name in TITLE_CLASSES for edit in EDITS for changed in (True, False)}
    for title, functions, unchanged in zip(matrix["titles"], matrix["functions"], matrix["unchanged"]):
        for name, belongs in TITLE_CLASSES.items():
            if belongs(title):
                for edit, same in zip(functions, unchanged):
                    count[(name, edit, not bool(same))] += 1
    print("\nclass      edit             changed  unchanged")
    for name in TITLE_CLASSES:
        for edit in EDITS:
            notes = [f"{'changed' if c else 'unchanged'}: {IMPOSSIBLE_CELLS[(name, edit, c)]}"
                     for c in (True, False) if (name, edit, c) in IMPOSSIBLE_CELLS]
            print(f"{name:10s} {edit:16s} {count[(name, edit, True)]:7d} {count[(name, edit, False)]:10d}  "
                  + "; ".join(notes))
    assert set(IMPOSSIBLE_CELLS) <= set(count) and len(count) == 48
    for cell, reason in IMPOSSIBLE_CELLS.items():
        if reason == NEVER:
            assert count[cell] == 0, cell
    short = {cell: n for cell, n in count.items() if cell not in IMPOSSIBLE_CELLS and n < MIN_PER_CELL}
    assert not short, short


def test_matrix_reaches_the_cut_the_second_strip_and_the_padding(matrix):
    grown = {256: 0, 257: 0}
    second_strip = padded = 0
    for title, functions, unchanged, edited, expected in zip(matrix["titles"], matrix["functions"], matrix["unchanged"],
                                                             matrix["edited"], matrix["expected"]):
        inserting = [f for f, same in zip(functions, unchanged) if f in ("add_letter", "add_space") and not same]
        if len(title) >= 253 and len(inserting) == 2 and len(edited) == len(title) + 2 and len(edited) in grown:
            grown[len(edited)] += 1                               # two inserting edits, then the cut
            assert len(expected) <= 255 and edited.startswith(expected)
        stripped = _collapsed(edited)
        if len(stripped) > 255 and stripped[254] == " ":          # the cut leaves a trailing space
            second_strip += 1
            assert expected == stripped[:254] and len(expected) < 255
        if len(stripped) < 3:
            padded += 1
            assert expected == "0" * (3 - len(stripped)) + stripped and len(expected) == 3
    print(f"\ngrown to 256: {grown[256]}, to 257: {grown[257]}; second strip: {second_strip}; padded: {padded}")
    assert grown[256] >= 3 and grown[257] >= 3 and second_strip >= 3 and padded >= 3
