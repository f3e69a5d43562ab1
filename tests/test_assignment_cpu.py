"""One-to-one matches without a GPU: the two restatements of tests/assignment_cases.py against each other and against the
definition of a stable matching, what every case claims to hold, the host functions of `prediction`, and the C ABI
surface with its argument errors (refused before the first HIP call)."""
import ctypes
import os
import re

import numpy as np
import pytest

import assignment_cases as ac
from doppel_speller_amd import _lib, prediction

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def solved():
    """Every case with its keys and its matching, computed once."""
    out = {}
    for name, make in ac.ALL.items():
        case = make()
        keys = ac.keys_of(case)
        out[name] = (case, keys, ac.deferred_acceptance(case.row, keys, case.n_truth))
    return out


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", sorted(ac.ALL))
def test_the_restatements_agree_and_the_result_is_stable(solved, name):
    case, keys, result = solved[name]
    assert ac.is_stable(case.row, keys, case.n_truth, result.match_row, result.match_slot)
    matched = result.match_row[result.match_row >= 0]
    assert np.unique(matched).shape[0] == matched.shape[0]
    if ac.is_descending(case.row, keys, case.n_truth):
        assert same(ac.greedy(case.row, keys, case.n_truth), result)
    else:
        assert name in ("unordered", "eligibility", "negative_threshold")
    rng = np.random.RandomState(11)
    for _ in range(5):
        assert same(ac.deferred_acceptance(case.row, keys, case.n_truth, rng.permutation(case.row.shape[0])), result)


def test_is_stable_refuses_what_is_not():
    case = ac.best_claimant()
    keys = ac.keys_of(case)
    # every row keeps its best claimant, once: q2 on t1, q1 on t0, q0 nowhere -- q0's key for t0 is above q1's
    assert not ac.is_stable(case.row, keys, 2, np.array([-1, 0, 1]), np.array([-1, 0, 0]))
    assert not ac.is_stable(case.row, keys, 2, np.array([1, 0, 1]), np.array([0, 0, 0]))          # t1 twice
    assert not ac.is_stable(case.row, keys, 2, np.array([0, -1, 1]), np.array([0, -1, 0]))        # the slot holds t1
    assert ac.is_stable(case.row, keys, 2, np.array([0, -1, 1]), np.array([1, -1, 0]))


def test_each_case_has_what_it_claims(solved):
    case, keys, result = solved["no_contention"]
    assert (result.match_slot == 0).all() and result.counts.tolist() == [3000, 1000, 0, 0]

    case, keys, result = solved["best_claimant"]
    assert result.match_row.tolist() == [0, -1, 1] and result.match_slot.tolist() == [1, -1, 0]
    assert result.counts.tolist() == [4, 2, 2, 1]

    case, keys, result = solved["chain"]
    length = case.row.shape[0] - 1
    assert length == 300 and result.match_slot.tolist() == [0] + [1] * length
    assert result.match_row.tolist() == list(range(length + 1)) and result.counts[2] >= length - 1
    scores = np.stack((case.probability[1:, 0], case.probability[1:, 1]), axis=1).reshape(-1)
    assert (np.diff(scores) < 0).all() and scores.min() > case.threshold

    case, keys, result = solved["classes"]
    assert np.nonzero(result.match_row >= 0)[0].tolist() == list(ac.CLASS_WINNERS)
    assert keys[0, 0] >> np.uint64(62) == 3 and keys[1, 0] >> np.uint64(62) == 2 and keys[2, 0] >> np.uint64(62) == 1
    assert case.probability[6, 0] == np.nextafter(case.probability[5, 0], np.float32(1))
    assert keys[6, 0] >> np.uint64(31) == (keys[5, 0] >> np.uint64(31)) + np.uint64(1)

    (case, slots), (_, keys, result) = ac.eligibility(), solved["eligibility"]
    assert result.match_slot.tolist() == slots.tolist()
    flat = case.probability[case.stage == 3]
    for value in (case.threshold, np.nextafter(case.threshold, np.float32(2)), np.nextafter(case.threshold, np.float32(-2))):
        assert (flat == value).any()
    assert np.isnan(flat).any() and (case.row == -1).any() and (case.row == case.n_truth).any() and (case.stage == 0).any()
    (case, slots), (_, keys, result) = ac.negative_threshold(), solved["negative_threshold"]
    assert result.match_slot.tolist() == slots.tolist() and case.threshold < 0
    assert np.signbit(case.probability[0, 0]) and case.probability[0, 0] == 0

    case, keys, result = solved["repeated_rows"]
    assert (keys[0] != 0).tolist() == [True, False, False, True] and result.match_row.tolist() == [1, 0]

    case, keys, result = solved["unordered"]
    assert not ac.is_descending(case.row, keys, case.n_truth)
    sorted_loop = ac.greedy(case.row[:2], keys[:2], case.n_truth)
    assert sorted_loop.match_row.tolist() == [1, -1] and result.match_row[:2].tolist() == [0, 1]
    assert not same(ac.greedy(case.row, keys, case.n_truth), result)

    case, keys, result = solved["hot_row"]
    assert ((case.row == 0) & (keys != 0)).sum() >= 5000 and (result.match_row == 0).sum() == 1
    assert (result.match_row >= 0).sum() == 65 and result.counts[3] > 4000

    case, keys, result = solved["random_ties"]
    assert case.row.shape == (20000, 5) and case.n_truth == 5000
    assert np.unique(case.probability[case.stage == 3]).shape[0] == 16
    assert {1, 2, 3} <= set((keys[keys != 0] >> np.uint64(62)).tolist())
    assert ac.is_descending(case.row, keys, case.n_truth) and result.counts[2] > 1000 and result.counts[3] > 100
    assert ((case.stage == 3) & (case.probability == case.threshold)).any()

    assert solved["no_title"][2].counts.tolist() == [0, 0, 0, 0] and solved["no_title"][2].match_row.shape == (0,)
    assert solved["odd_count"][0].row.shape[0] % 64 != 0 and (solved["n_truth_1"][2].match_row >= 0).sum() == 1


def test_edge_keys_number_the_titles_of_the_whole_call():
    case = ac.random_ties(count=500, n_truth=200)
    whole = ac.keys_of(case)
    parts = [ac.edge_keys(*chunk[1:], chunk[0], case.n_truth, case.threshold) for chunk in ac.cut(case, (7, 300, 499))]
    assert np.array_equal(np.concatenate(parts), whole)
    edges = whole != 0
    assert np.array_equal((whole & np.uint64(ac.TITLE_MASK))[edges],
                          (ac.TITLE_MASK - np.nonzero(edges)[0]).astype(np.uint64))


# ---- the host functions of prediction ------------------------------------------------------------------------------------

def test_assignment_frame():
    case = ac.best_claimant()
    result = ac.expected(case)
    ids = np.array([70, 50], dtype=np.int64)
    frame = prediction.assignment_frame(np.array([12, 11, 10]), result.match_row, result.match_slot, result.first_row,
                                        case.row, case.probability, case.ratio, case.stage, ids)
    assert tuple(frame.columns) == prediction.ASSIGNMENT_COLUMNS
    assert [str(t) for t in frame.dtypes] == ["int64", "int64", "int64", "int8", "float32", "uint8", "int64", "int64", "bool"]
    assert frame["test_index"].tolist() == [12, 11, 10] and frame["match_row"].tolist() == [0, -1, 1]
    assert frame["title_id"].tolist() == [70, -1, 50] and frame["stage"].tolist() == [3, 0, 3]
    assert frame["rank"].tolist() == [2, 0, 1] and frame["first_choice_row"].tolist() == [1, 0, 1]
    assert frame["displaced"].tolist() == [True, True, False] and frame["levenshtein_ratio"].tolist() == [50, 0, 50]
    assert frame["probability"].to_numpy()[[0, 2]].tolist() == [np.float32(0.95), np.float32(0.995)]
    assert np.isnan(frame["probability"].to_numpy()[1])
    with pytest.raises(ValueError, match="match_slot"):
        prediction.assignment_frame(np.arange(3), result.match_row, np.array([0, -1, 0]), result.first_row, case.row,
                                    case.probability, case.ratio, case.stage, ids)
    empty = prediction.assignment_frame(np.zeros(0, np.int64), *(np.zeros(0, np.int32),) * 3,
                                        *(np.zeros((0, 2), d) for d in (np.int32, np.float32, np.uint8, np.int8)), ids)
    assert len(empty) == 0 and empty.dtypes.tolist() == frame.dtypes.tolist()


def test_validate_assignment_and_the_memory_it_asks_for():
    assert prediction.validate_assignment(5, 100, 0.9) == (5, 0.9)
    assert prediction.validate_assignment(np.int64(1), 1, np.float32(0.5)) == (1, 0.5)
    for n in (0, -1, 101, True, 2.0, None):
        with pytest.raises(ValueError, match="n "):
            prediction.validate_assignment(n, 100, 0.9)
    for threshold in (float("nan"), float("inf"), 1e39, "0.9", None, True):
        with pytest.raises(ValueError, match="probability_threshold"):
            prediction.validate_assignment(5, 100, threshold)
    assert prediction.assignment_bytes(100_000, 5, 500_000) == 12 * 500_000 + 8 * 500_000 + 16 * 100_000
    assert prediction.ASSIGNMENT_COUNTS == ("edges", "matched", "displaced", "displaced_unmatched", "proposals", "rounds")


def test_package_exports():
    import doppel_speller_amd as ds
    assert ds.ASSIGNMENT_COLUMNS == prediction.ASSIGNMENT_COLUMNS and ds.ASSIGNMENT_COUNTS == prediction.ASSIGNMENT_COUNTS
    assert ds.assignment_frame is prediction.assignment_frame and ds.validate_assignment is prediction.validate_assignment
    assert callable(ds.Prediction.one_to_one_matches) and "one_to_one_matches" in ds.__doc__
    assert callable(ds.CandidatePipeline.enqueue_assign_edges)
    assert "predict.py:158-161" in ds.Prediction.one_to_one_matches.__doc__


# ---- the C ABI surface ------------------------------------------------------------------------------------------------------

def test_header_declares_what_the_binding_calls():
    header = open(os.path.join(ROOT, "include", "doppel_amd.h")).read()

    def types_of(name):
        declaration = re.search(r"int %s\(([^;]*)\);" % name, header)
        assert declaration, f"{name} is not declared"
        arguments = [a.strip() for a in declaration.group(1).replace("\n", " ").split(",")]
        return [a.rsplit(" ", 1)[0] + ("*" if a.rsplit(" ", 1)[1].startswith("*") else "") for a in arguments]

    assert types_of("ds_assign_edges_device") == [
        "const int32_t*", "const float*", "const uint8_t*", "const int8_t*", "int64_t", "int64_t", "int64_t", "int32_t",
        "int64_t", "float", "uint64_t*", "int32_t*", "void*"]
    assert types_of("ds_assign_solve_device") == [
        "const int32_t*", "const uint64_t*", "int64_t", "int32_t", "int64_t", "uint64_t*", "int32_t*", "int32_t*", "int32_t*",
        "int32_t*", "int64_t*", "void*"]
    assert re.search(r"int ds_assign_option\(const char \*name, int64_t value\);", header)
    assert "SYNCHRONISES `stream`" in header
    assert {"ds_assign_edges_device", "ds_assign_solve_device", "ds_assign_option"} <= set(_lib.EXPORTED_SYMBOLS)
    assert "ds_assign.hip" in _lib._SOURCES


@pytest.fixture(scope="module")
def library():
    """The library with the binding's argument types, loaded without asking for a device."""
    import doppel_speller_amd as ds
    return _lib._declare(ctypes.CDLL(ds.build_library()))


def test_argument_errors_need_no_device(library):
    """Every bad argument is refused before the first HIP call: the pointers here are never dereferenced."""
    some, null = ctypes.c_void_p(0x1000), ctypes.c_void_p(0)
    edges = library.ds_assign_edges_device
    good = [some, some, some, some, 0, 8, 8, 5, 100, 0.9, some, some, null]
    for position in (0, 1, 2, 3, 10, 11):
        bad = list(good)
        bad[position] = null
        assert edges(*bad) == -1 and b"null" in library.ds_last_error(), position
    for position, value, word in ((4, -1, b"negative"), (5, -1, b"negative"), (6, -1, b"negative"), (7, 0, b"positive"),
                                  (7, -3, b"positive"), (8, -1, b"n_truth"), (8, 1 << 31, b"n_truth"),
                                  (6, 1 << 31, b"below 2^31"), (9, float("nan"), b"finite"), (9, float("inf"), b"finite"),
                                  (9, float("-inf"), b"finite"), (5, 9, b"not among"), (4, 1, b"not among"),
                                  (4, 9, b"not among")):
        bad = list(good)
        bad[position] = value
        assert edges(*bad) == -1 and word in library.ds_last_error(), (position, value, library.ds_last_error())
    empty = list(good)
    empty[5] = 0
    assert edges(*empty) == 0                                      # nothing to do: no launch, no device needed
    empty[4] = 8
    assert edges(*empty) == 0

    solve = library.ds_assign_solve_device
    good = [some, some, 8, 5, 100, some, some, some, some, some, some, null]
    for position in (0, 1, 5, 6, 7, 8, 9, 10):
        bad = list(good)
        bad[position] = null
        assert solve(*bad) == -1 and b"null" in library.ds_last_error(), position
    for position, value, word in ((2, -1, b"negative"), (2, 1 << 31, b"below 2^31"), (3, 0, b"positive"),
                                  (4, -1, b"n_truth"), (4, 1 << 31, b"n_truth")):
        bad = list(good)
        bad[position] = value
        assert solve(*bad) == -1 and word in library.ds_last_error(), (position, value, library.ds_last_error())

    option = library.ds_assign_option
    assert option(b"max_blocks", -1) == -1 and option(b"max_blocks", (1 << 20) + 1) == -1
    assert option(b"rounds_per_sync", 0) == -1 and option(b"rounds_per_sync", 1025) == -1
    assert option(b"no_such_option", 1) == -1 and option(None, 1) == -1
    assert option(b"max_blocks", 1) == 0 and option(b"max_blocks", 1 << 20) == 0 and option(b"max_blocks", 0) == 0
    assert option(b"rounds_per_sync", 1) == 0 and option(b"rounds_per_sync", 1024) == 0
    assert option(b"rounds_per_sync", 8) == 0
