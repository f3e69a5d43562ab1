"""Ranked matches without a GPU: the NumPy restatement of the ranking rule (tests/ranked_cases.py) against a plain-Python
transcription with sorted(), ranked_matches' argument checks, the frame it builds, and the C ABI surface."""
import os
import re

import numpy as np
import pytest

import ranked_cases as rc
from doppel_speller_amd import _lib, prediction

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _slots(k):
    return sorted({1, max(1, k // 2), k})


@pytest.mark.parametrize("ties", ["none", "some", "all", "k"])
@pytest.mark.parametrize("k", [1, 2, 5, 17, 64, 100])
def test_restatement_equals_the_sorted_transcription(k, ties):
    n_truth = 2 * k + 2
    groups = rc.make_groups(48, k, n_truth, seed=1000 + k, ties=ties)
    for n in _slots(k):
        assert rc.as_lists(rc.rank_matches(*groups, n, n_truth)) == rc.rank_matches_python(*groups, n, n_truth), n
    rows, probabilities, ratios, exact, best = groups
    for exact_, best_ in ((None, best), (exact, None), (None, None)):
        assert rc.as_lists(rc.rank_matches(rows, probabilities, ratios, exact_, best_, k, n_truth)) == \
            rc.rank_matches_python(rows, probabilities, ratios, exact_, best_, k, n_truth)


def test_crafted_groups():
    rows = np.array([[4, 9, 2, 7, -1], [4, 9, 2, 7, 30], [4, 9, 2, 7, 5], [4, 9, 2, 7, 5]], dtype=np.int32)
    probabilities = np.array([[.5, .75, .75, .25, 1.], [.5, .5, .5, .5, .5], [.1, .2, .3, .4, .5], [0., 0., 1., 0., 0.]],
                             dtype=np.float32)
    ratios = np.array([[10, 20, 30, 40, 50]] * 4, dtype=np.uint8)
    exact = np.array([-1, 7, 11, -1], dtype=np.int32)
    best = np.array([-1, 7, 11, 9], dtype=np.int32)
    row, probability, ratio, stage = rc.rank_matches(rows, probabilities, ratios, exact, best, 5, 12)
    # query 0: no head, the tie of rows 9 and 2 in candidate order, the row -1 skipped, one empty slot
    assert row[0].tolist() == [9, 2, 4, 7, -1] and stage[0].tolist() == [3, 3, 3, 3, 0]
    assert ratio[0].tolist() == [20, 30, 10, 40, 0] and np.isnan(probability[0, 4])
    assert probability[0, :4].tolist() == [.75, .75, .5, .25]
    # query 1: exact head among the candidates with its own ratio, all equal: candidate order, row 30 >= n_truth skipped
    assert row[1].tolist() == [7, 4, 9, 2, -1] and stage[1].tolist() == [1, 3, 3, 3, 0]
    assert ratio[1].tolist() == [40, 10, 20, 30, 0] and probability[1, 0] == 1.0
    # query 2: exact head outside the candidates: ratio 100, then the five candidates cut to four
    assert row[2].tolist() == [11, 5, 7, 2, 9] and ratio[2].tolist() == [100, 50, 40, 30, 20]
    # query 3: close head
    assert row[3].tolist() == [9, 2, 4, 7, 5] and stage[3].tolist() == [2, 3, 3, 3, 3] and ratio[3, 0] == 20
    cut = rc.rank_matches(rows, probabilities, ratios, exact, best, 1, 12)
    assert cut[0][:, 0].tolist() == [9, 7, 11, 9] and cut[3][:, 0].tolist() == [3, 1, 1, 2]
    assert rc.as_lists((row, probability, ratio, stage)) == rc.rank_matches_python(rows, probabilities, ratios, exact,
                                                                                   best, 5, 12)


@pytest.fixture
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the library was touched before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", refuse)


@pytest.mark.parametrize("n", [0, -1, True, False, 2.0, "3", None, 11, np.int64(0)])
def test_bad_n_is_refused_before_any_device_work(no_library, n):
    p = prediction.Prediction.__new__(prediction.Prediction)
    p.top_n = 10
    with pytest.raises(ValueError, match="^n "):
        p.ranked_matches(["a title"], n=n)
    with pytest.raises(ValueError, match="^n "):
        prediction.validate_rank(n, 10)


def test_good_n_and_bad_test_index(no_library):
    assert prediction.validate_rank(1, 10) == 1 and prediction.validate_rank(np.int32(10), 10) == 10
    p = prediction.Prediction.__new__(prediction.Prediction)
    p.top_n = 10
    with pytest.raises(ValueError, match="test indexes"):
        p.ranked_matches(["a", "b"], n=3, test_index=[1, 1])
    with pytest.raises(ValueError, match="2 titles but 1 test indexes"):
        p.ranked_matches(["a", "b"], n=3, test_index=[1])


def test_ranked_frame():
    ids = np.array([100, 101, 102, 103], dtype=np.int64)
    rows = np.array([[2, 0, -1], [-1, -1, -1], [3, 1, 0]], dtype=np.int32)
    probabilities = np.array([[1., .5, np.nan], [np.nan] * 3, [.9, .9, .1]], dtype=np.float32)
    ratios = np.array([[100, 40, 0], [0, 0, 0], [70, 60, 50]], dtype=np.uint8)
    stages = np.array([[1, 3, 0], [0, 0, 0], [3, 3, 3]], dtype=np.int8)
    frame = prediction.ranked_frame([7, 5, 3], rows, probabilities, ratios, stages, ids)
    assert tuple(frame.columns) == prediction.RANKED_COLUMNS
    assert frame["test_index"].tolist() == [3, 3, 3, 7, 7] and frame["rank"].tolist() == [1, 2, 3, 1, 2]
    assert frame["match_row"].tolist() == [3, 1, 0, 2, 0] and frame["title_id"].tolist() == [103, 101, 100, 102, 100]
    assert frame["levenshtein_ratio"].tolist() == [70, 60, 50, 100, 40] and frame["stage"].tolist() == [3, 3, 3, 1, 3]
    assert frame["probability"].dtype == np.float32 and not frame["probability"].isna().any()
    empty = prediction.ranked_frame(np.zeros(0, np.int64), *(a[:0] for a in (rows, probabilities, ratios, stages)), ids)
    assert tuple(empty.columns) == prediction.RANKED_COLUMNS and len(empty) == 0
    assert empty.dtypes.tolist() == frame.dtypes.tolist()


def test_header_declares_what_the_binding_calls():
    header = open(os.path.join(ROOT, "include", "doppel_amd.h")).read()
    declaration = re.search(r"int ds_rank_matches_device\(([^;]*)\);", header)
    assert declaration, "ds_rank_matches_device is not declared"
    arguments = [a.strip() for a in declaration.group(1).replace("\n", " ").split(",")]
    assert [a.rsplit(" ", 1)[0] for a in arguments] == [
        "const int32_t", "const float", "const uint8_t", "const int32_t", "const int32_t", "int64_t", "int32_t", "int32_t",
        "int64_t", "int32_t", "float", "uint8_t", "int8_t", "void"]
    assert [a.rsplit(" ", 1)[1].startswith("*") for a in arguments] == [True] * 5 + [False] * 4 + [True] * 5
    assert re.search(r"int ds_rank_option\(const char \*name, int64_t value\);", header)
    assert {"ds_rank_matches_device", "ds_rank_option"} <= set(_lib.EXPORTED_SYMBOLS)
    assert "ds_rank.hip" in _lib._SOURCES


def test_package_exports():
    import doppel_speller_amd as ds
    assert ds.Candidates is prediction.Candidates and ds.RANKED_COLUMNS == prediction.RANKED_COLUMNS
    assert ds.validate_rank is prediction.validate_rank
