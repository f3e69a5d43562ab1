"""Prediction (doppel-speller_amd/prediction.py) without a GPU: argument validation before any library call, the host
finaliser and stage combination, and the query rows it derives against a truth-only vocabulary."""
import numpy as np
import pytest

from doppel_speller_amd import _lib, prediction
from doppel_speller_amd.prediction import Prediction


@pytest.fixture
def no_library(monkeypatch):
    """Any library call fails the test: validation must happen first."""
    def refuse():
        raise AssertionError("the library was called before the arguments were validated")
    monkeypatch.setattr(_lib, "lib", refuse)


def test_duplicate_truth_ids_are_refused(no_library):
    with pytest.raises(ValueError, match="unique"):
        Prediction(["abc", "abd", "abe"], [4, 5, 4], object(), top_n=1)


def test_length_mismatch_is_refused(no_library):
    with pytest.raises(ValueError, match="2 title ids"):
        Prediction(["abc", "abd", "abe"], [1, 2], object(), top_n=1)


def test_negative_id_is_refused(no_library):
    with pytest.raises(ValueError, match="non-negative"):
        Prediction(["abc", "abd"], [0, -1], object(), top_n=1)


@pytest.mark.parametrize("chunk", [0, -5, 2.5, True])
def test_bad_chunk_queries_is_refused(no_library, chunk):
    with pytest.raises(ValueError, match="chunk_queries"):
        Prediction(["abc", "abd"], [0, 1], object(), top_n=1, chunk_queries=chunk)


def test_top_n_beyond_the_truth_set_is_refused(no_library):
    with pytest.raises(ValueError, match="top_n"):
        Prediction(["abc", "abd"], [0, 1], object(), top_n=3)


@pytest.mark.parametrize("title", ["", "   ", "\t \n"])
def test_empty_single_title_is_refused(no_library, title):
    p = Prediction.__new__(Prediction)        # no truth side needed: the title is checked first (cli.py:75-76)
    with pytest.raises(ValueError, match="empty"):
        p.closest_search_single_title(title)


def test_test_index_validation(no_library):
    assert np.array_equal(prediction.validate_queries(["a", "b"], None), [0, 1])
    with pytest.raises(ValueError, match="unique"):
        prediction.validate_queries(["a", "b"], [3, 3])
    with pytest.raises(ValueError, match="test indexes"):
        prediction.validate_queries(["a", "b"], [3])


def test_stage_priority():
    exact = np.array([5, -1, -1, -1, 7])
    close = np.array([6, 2, -1, -1, 8])
    model = np.array([1, 1, 3, -1, 9])
    rows, stages = prediction.combine_stages(exact, close, model)
    assert rows.tolist() == [5, 2, 3, -1, 7]
    assert stages.tolist() == [prediction.STAGE_EXACT, prediction.STAGE_CLOSE, prediction.STAGE_MODEL,
                               prediction.STAGE_NONE, prediction.STAGE_EXACT]


def test_finaliser_sorts_by_test_index_and_fills_not_found():
    ids = np.array([100, 101, 102, 103], dtype=np.int64)
    test_index = np.array([30, 10, 20, 0])
    rows = np.array([3, -1, 0, -1])
    out = prediction.finalize_output(test_index, rows, ids)
    assert list(out.columns) == ["title_id", "test_index"]
    assert out["test_index"].tolist() == [0, 10, 20, 30]
    assert out["title_id"].tolist() == [-1, -1, 100, 103]


def test_query_rows_match_the_native_build_of_both_collections():
    """query_rows against the truth-only vocabulary == the query rows of ds_problem_create(truth, queries), columns
    renumbered: same q_maxint bits, same truth columns in the same order."""
    from doppel_speller_amd import synth
    from doppel_speller_amd.match_maker import NativeProblem
    w = synth.make_workload(3000, 400, seed=5)
    truth = synth._to_strings(w.t_flat, w.t_off)
    queries = synth._to_strings(w.q_flat, w.q_off) + ["zzzqqq", "ab", "x y", truth[0]]
    t_chars, t_offsets = prediction._pack(truth)
    q_chars, q_offsets = prediction._pack(queries)
    alone = NativeProblem.from_flat(t_chars, t_offsets, np.zeros(1, np.uint8), np.zeros(1, np.int64), 3).arrays()
    both = NativeProblem.from_flat(t_chars, t_offsets, q_chars, q_offsets, 3).arrays()
    rowptr, cols, maxint = prediction.query_rows(q_chars, q_offsets, alone["vocabulary_keys"], alone["idf32"],
                                                 alone["idf64"])
    assert np.array_equal(maxint.view(np.uint64), both["q_maxint"].view(np.uint64))
    assert np.array_equal(alone["sums32"].view(np.uint32), both["sums32"].view(np.uint32))
    keys = alone["vocabulary_keys"]
    renumber = np.searchsorted(keys, both["vocabulary_keys"])
    in_truth = renumber < keys.shape[0]
    in_truth[in_truth] = keys[renumber[in_truth]] == both["vocabulary_keys"][in_truth]
    for q in range(len(queries)):
        union = both["q_cols"][both["q_rowptr"][q]:both["q_rowptr"][q + 1]]
        assert np.array_equal(renumber[union][in_truth[union]], cols[rowptr[q]:rowptr[q + 1]]), q
