"""The threshold sweep without a GPU: predictions_accuracy against a transcription of the reference's loop, the close ratio
read from its three parts against oracle.close_ratios at every threshold, the crafted queries of tests/sweep_cases.py
against what they were written to get, threshold_sweep's argument checks and frame, and the C ABI surface."""
import os
import re

import numpy as np
import pytest

import sweep_cases as sc
import title_cases as tc
from doppel_speller_amd import _lib, prediction
from doppel_speller_amd.feature_engineering import SORT_KEY

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cli_loop(predicted, actual):
    """cli.py:107-128, on {test_index: title_id} dicts as the command builds them."""
    actual = dict(enumerate(actual))
    predictions = dict(enumerate(predicted))
    correctly_matched_existing, correctly_matched_non_existing = 0, 0
    incorrectly_matched_existing, incorrectly_matched_non_existing = 0, 0
    for key, actual_value in actual.items():
        prediction_value = predictions[key]
        if prediction_value == -1:
            if actual_value == prediction_value:
                correctly_matched_non_existing += 1
            else:
                incorrectly_matched_non_existing += 1
        else:
            if actual_value == prediction_value:
                correctly_matched_existing += 1
            else:
                incorrectly_matched_existing += 1
    return {"correctly_matched": correctly_matched_existing, "incorrectly_matched": incorrectly_matched_existing,
            "correctly_not_found": correctly_matched_non_existing,
            "incorrectly_not_found": incorrectly_matched_non_existing,
            "custom_error": incorrectly_matched_non_existing + (incorrectly_matched_existing * 5)}


def test_predictions_accuracy_is_the_loop_of_the_reference():
    predicted = np.array([5, 5, -1, -1, 9, 0, -1, 3], dtype=np.int64)
    actual = np.array([5, 6, -1, 7, -1, 0, -1, 3], dtype=np.int64)
    got = prediction.predictions_accuracy(predicted, actual)
    assert got == _cli_loop(predicted.tolist(), actual.tolist())
    assert got == {"correctly_matched": 3, "incorrectly_matched": 2, "correctly_not_found": 2,
                   "incorrectly_not_found": 1, "custom_error": 11}
    assert list(got) == list(prediction.SWEEP_COLUMNS[2:]) and all(type(v) is int for v in got.values())
    nothing = np.full(8, -1, dtype=np.int64)
    assert prediction.predictions_accuracy(nothing, actual) == _cli_loop(nothing.tolist(), actual.tolist())
    assert prediction.predictions_accuracy(predicted, nothing) == _cli_loop(predicted.tolist(), nothing.tolist())
    assert prediction.predictions_accuracy(nothing, nothing)["correctly_not_found"] == 8
    rng = np.random.RandomState(3)
    for _ in range(20):
        a, b = rng.randint(-1, 4, 50), rng.randint(-1, 4, 50)
        assert prediction.predictions_accuracy(a, b) == _cli_loop(a.tolist(), b.tolist())
    assert prediction.predictions_accuracy([], [])["custom_error"] == 0
    with pytest.raises(ValueError, match="3 predicted ids but 2 actual ids"):
        prediction.predictions_accuracy([1, 2, 3], [1, 2])


@pytest.fixture(scope="module")
def parts(oracle):
    case = tc.close_case()
    pair_q, pair_t = sc.close_pairs(case)
    return case, pair_q, pair_t, sc.case_parts(oracle, case, pair_q, pair_t, SORT_KEY)


def test_three_parts_give_the_ratio_at_every_threshold(oracle, parts):
    case, pair_q, pair_t, (d, r, s) = parts
    for t in range(101):
        expected = tc.expected_ratios(oracle, case, pair_q, pair_t, t, SORT_KEY)
        assert np.array_equal(sc.value_at(d, r, s, t), expected), t
    # what the pairs hold: two empty titles, titles past 64 characters on both sides, a token sort that changes the ratio
    valid = tc.valid_pairs(case, pair_q, pair_t)
    lq, lt = case.q_len[np.where(valid, pair_q, 0)], case.t_len[np.where(valid, pair_t, 0)]
    assert (valid & (lq == 0) & (lt == 0)).sum() >= 4 and (d[valid & (lq == 0) & (lt == 0)] == 100).all()
    assert (valid & (lq > 64) & (lt > 64) & (d >= 94)).sum() >= 5
    assert (valid & (s > r) & (r <= d) & (s > 94)).sum() >= 5
    assert (~valid).sum() >= 100 and not d[~valid].any() and not r[~valid].any() and not s[~valid].any()


def test_skipped_parts_read_the_same_inside_their_range(parts):
    _, _, _, (d, r, s) = parts
    for t_min, t_max in ((0, 100), (94, 94), (50, 90)):
        kept = sc.skipped_parts(d, r, s, t_min, t_max)
        for t in range(t_min, t_max + 1):
            assert np.array_equal(sc.value_at(*kept, t), sc.value_at(d, r, s, t)), (t_min, t_max, t)
    at_94 = sc.skipped_parts(d, r, s, 94, 94)
    assert (at_94[1] == 0).sum() > (r == 0).sum() and (at_94[2] == 0).sum() > (s == 0).sum()


def test_crafted_queries_get_what_they_were_written_for(oracle):
    lev, prob = sc.GRID_3X7
    for k in (5, 100):
        rows, d, r, s, p, exact, actual = sc.crafted_queries(k)
        got = sc.predictions_of(oracle, rows, d, r, s, p, exact, lev, prob)
        assert got.shape == (3, 7, sc.CRAFTED)
        model_6 = [rows[6, 1]] * 4 + [-1] * 3
        for u in range(7):
            below_80, below_50 = u < 4, u < 2
            assert got[:, u, 0].tolist() == [77, 77, 77]
            assert got[:, u, 1].tolist() == [rows[1, 2] if below_80 else -1] * 3
            assert got[:, u, 2].tolist() == [rows[2, 1], rows[2, 0], rows[2, 0]]
            assert got[:, u, 3].tolist() == [-1, -1, -1]
            assert got[:, u, 4].tolist() == [rows[4, 0] if below_50 else -1] * 3
            assert got[:, u, 5].tolist() == [rows[5, 3]] * 3
            assert got[:, u, 6].tolist() == [rows[6, 0], model_6[u], model_6[u]]
        counts = sc.count_outcomes(got, actual)
        assert counts[0, 0].tolist() == [3, 3, 1, 0] and counts[2, 6].tolist() == [2, 1, 1, 3]
        assert (counts.sum(axis=-1) == sc.CRAFTED).all()


@pytest.fixture
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the library was touched before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", refuse)


IDS = np.array([40, 10, 30, 20], dtype=np.int64)


def test_validate_sweep_normalises(no_library):
    lev, prob, shown, actual = prediction.validate_sweep([94, 10, 94, 100, 0], [0.9, 0.5, 0.9, np.float32(0.9), 0.25],
                                                         [10, -1, 20, 40], IDS, 4)
    assert lev.dtype == np.int32 and lev.tolist() == [0, 10, 94, 100]
    assert prob.dtype == np.float32 and prob.tolist() == [0.25, 0.5, np.float32(0.9)]
    assert shown.dtype == np.float64 and shown.tolist() == [0.25, 0.5, 0.9]
    assert actual.dtype == np.int32 and actual.tolist() == [1, -1, 3, 0]
    lev, prob, _, _ = prediction.validate_sweep(np.arange(101)[::-1], np.linspace(0, 1, 256), [], IDS, 0)
    assert lev.shape == (101,) and prob.shape == (256,) and (np.diff(lev) > 0).all() and (np.diff(prob) > 0).all()
    assert prediction.validate_sweep(np.arange(101).tolist() * 2, [1, 0], [], IDS, 0)[1].tolist() == [0.0, 1.0]


@pytest.mark.parametrize("lev, prob, actual, message", [
    ([101], [0.9], [10], r"\[0, 100\]"), ([-1], [0.9], [10], r"\[0, 100\]"), ([], [0.9], [10], "one at least"),
    ([94.0], [0.9], [10], "integers"), ([True], [0.9], [10], "integers"), ([[94]], [0.9], [10], "one-dimensional"),
    ([94], [np.nan], [10], "finite"), ([94], [np.inf], [10], "finite"), ([94], [1e300], [10], "finite"),
    ([94], [], [10], "one at least"), ([94], ["0.9"], [10], "numbers"), ([94], [[0.9]], [10], "one-dimensional"),
    ([94], np.linspace(0, 1, 257), [10], "256 at most"),
    ([94], [0.9], [11], "actual title id 11 is neither -1 nor an id"), ([94], [0.9], [-2], "actual title id -2"),
    ([94], [0.9], [41], "actual title id 41"), ([94], [0.9], [10.0], "integers"), ([94], [0.9], [10, 20], "1 titles but 2"),
])
def test_validate_sweep_refuses(no_library, lev, prob, actual, message):
    with pytest.raises(ValueError, match=message):
        prediction.validate_sweep(lev, prob, actual, IDS, 1)
    p = prediction.Prediction.__new__(prediction.Prediction)
    p.truth_title_ids, p.levenshtein_threshold, p.probability_threshold = IDS, 94, 0.9
    with pytest.raises(ValueError, match=message):
        p.threshold_sweep(["a title"], actual, lev, prob)


def test_more_thresholds_than_the_kernel_takes_cannot_be_named(no_library):
    # 101 integers in [0, 100] at the most exist: the limit of T holds by the range
    assert prediction.SWEEP_MAX_LEVENSHTEIN == 101 and prediction.SWEEP_MAX_PROBABILITY == 256
    assert prediction.validate_sweep(list(range(101)) + [50], [0.5], [], IDS, 0)[0].shape == (101,)
    p = prediction.Prediction.__new__(prediction.Prediction)
    p.truth_title_ids, p.levenshtein_threshold, p.probability_threshold = IDS, 94, 0.9
    with pytest.raises(ValueError, match="test indexes"):
        p.threshold_sweep(["a", "b"], [10, 20], test_index=[1, 1])
    with pytest.raises(ValueError, match="actual title id 11"):
        p.evaluate(["a"], [11])


def test_sweep_frame():
    counts = np.arange(2 * 3 * 4, dtype=np.int64).reshape(2, 3, 4)
    frame = prediction.sweep_frame(np.array([90, 94], np.int32), np.array([0.1, 0.5, 0.9]), counts.reshape(-1))
    assert tuple(frame.columns) == prediction.SWEEP_COLUMNS and len(frame) == 6
    assert frame["levenshtein_threshold"].tolist() == [90, 90, 90, 94, 94, 94]
    assert frame["probability_threshold"].tolist() == [0.1, 0.5, 0.9] * 2
    assert frame["correctly_matched"].tolist() == [0, 4, 8, 12, 16, 20]
    assert frame["incorrectly_not_found"].tolist() == [3, 7, 11, 15, 19, 23]
    assert frame["custom_error"].tolist() == [3 + 5 * 1, 7 + 5 * 5, 11 + 5 * 9, 15 + 5 * 13, 19 + 5 * 17, 23 + 5 * 21]
    assert frame.dtypes.tolist() == [np.int64, np.float64] + [np.int64] * 5


def test_header_declares_what_the_binding_calls():
    header = open(os.path.join(ROOT, "include", "doppel_amd.h")).read()

    def types_of(name):
        declaration = re.search(r"int %s\(([^;]*)\);" % name, header)
        assert declaration, f"{name} is not declared"
        arguments = [a.strip() for a in declaration.group(1).replace("\n", " ").split(",")]
        return [a.rsplit(" ", 1)[0] + ("*" if a.rsplit(" ", 1)[1].startswith("*") else "") for a in arguments]

    assert types_of("ds_close_parts_device") == [
        "ds_titles*", "ds_titles*", "const int32_t*", "int64_t", "int32_t", "int64_t", "uint8_t", "const uint8_t*",
        "int32_t", "int32_t", "uint8_t*", "uint8_t*", "uint8_t*", "void*"]
    assert types_of("ds_threshold_sweep_device") == [
        "const int32_t*", "const uint8_t*", "const uint8_t*", "const uint8_t*", "const float*", "const int32_t*",
        "const int32_t*", "int64_t", "int32_t", "const int32_t*", "int32_t", "const float*", "int32_t", "int64_t*", "void*"]
    assert re.search(r"int ds_sweep_option\(const char \*name, int64_t value\);", header)
    assert {"ds_close_parts_device", "ds_threshold_sweep_device", "ds_sweep_option"} <= set(_lib.EXPORTED_SYMBOLS)
    assert "ds_sweep.hip" in _lib._SOURCES


def test_package_exports():
    import doppel_speller_amd as ds
    assert ds.SWEEP_COLUMNS == prediction.SWEEP_COLUMNS and ds.predictions_accuracy is prediction.predictions_accuracy
    assert ds.validate_sweep is prediction.validate_sweep
    for name in ("threshold_sweep", "evaluate"):
        assert callable(getattr(ds.Prediction, name))
    for name in ("enqueue_close_parts", "close_parts", "enqueue_threshold_sweep"):
        assert callable(getattr(ds.CandidatePipeline, name))
