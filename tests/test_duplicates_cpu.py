"""The duplicate-groups stage without a GPU: the restatement of tests/duplicates_cases.py on hand-written cases with known
answers, validate_duplicates and duplicate_frame, the links frame, and the C ABI surface with its argument errors (which
are found before anything touches a device)."""
import ctypes
import os
import re

import numpy as np
import pytest

import duplicates_cases as dc
from doppel_speller_amd import _lib, prediction

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement ------------------------------------------------------------------------------------------------

def test_links_of_a_hand_written_call():
    rows = np.array([[1, 7, 5], [0, 9, -1], [6, 6, 3]], dtype=np.int32)           # queries are rows 5, 6, 7 of 9
    ratios = np.array([[95, 94, 100], [0, 100, 100], [96, 0, 0]], dtype=np.uint8)
    p = np.array([[0.95, 0.95, 1.0], [0.9, 1.0, 1.0], [np.nan, 0.91, 0.5]], dtype=np.float32)
    exact = np.array([8, -1, 7], dtype=np.int32)
    edges, reasons, counts = dc.links_of(rows, ratios, p, exact, 5, 9, 94, 0.9)
    assert reasons.tolist() == [[3, 2, 0], [0, 0, 0], [1, 2, 0]]                  # own row, row 9 and -1 are skipped
    assert edges.tolist() == [[5, 8], [5, 1], [5, 7], [7, 6], [7, 6]]             # exact first; row 7's exact is itself
    assert counts.tolist() == [1, 2, 2]
    assert reasons.dtype == np.uint8 and edges.dtype == np.int64 and counts.dtype == np.int64
    # no predictions, no exact rows: the close links alone
    edges, reasons, counts = dc.links_of(rows, ratios, None, None, 5, 9, 94, 0.9)
    assert reasons.tolist() == [[1, 0, 0], [0, 0, 0], [1, 0, 0]] and edges.tolist() == [[5, 1], [7, 6]]
    assert counts.tolist() == [0, 2, 0]
    # the thresholds are strict, the probability compares as float32
    assert dc.links_of(rows, ratios, p, None, 5, 9, 95, 0.95)[1].tolist() == [[0, 0, 0], [0, 0, 0], [1, 0, 0]]
    assert dc.links_of(rows, ratios, p, None, 5, 9, 100, float(np.float32(0.9)) - 1e-12)[1].tolist() == \
        [[2, 2, 0], [0, 0, 0], [0, 2, 0]]


def test_components_known_answers():
    labels, sizes = dc.components(8, [[5, 3], [7, 5], [2, 6], [3, 7], [4, 4]])
    assert labels.tolist() == [0, 1, 2, 3, 4, 3, 2, 3] and sizes.tolist() == [1, 1, 2, 3, 1, 3, 2, 3]
    assert labels.dtype == np.int32 and sizes.dtype == np.int32
    labels, sizes = dc.components(3, np.zeros((0, 2), dtype=np.int64))
    assert labels.tolist() == [0, 1, 2] and sizes.tolist() == [1, 1, 1]
    labels, sizes = dc.components(5, [[4, 3], [3, 2], [2, 1], [1, 0]])
    assert labels.tolist() == [0] * 5 and sizes.tolist() == [5] * 5


def test_the_builders_give_what_they_were_written_for():
    for order in ("ascending", "descending", "shuffled"):
        labels, sizes, _, counts = dc.expected(dc.chain(1000, order), 1000, dc.T, dc.U)
        assert not labels.any() and (sizes == 1000).all() and counts.tolist() == [0, 999, 0], order
    for centre in (0, 499):
        labels, sizes, _, counts = dc.expected(dc.star(500, centre), 500, dc.T, dc.U)
        assert not labels.any() and (sizes == 500).all() and counts.tolist() == [0, 499, 0]
    calls = dc.two_halves_joined_later(300)
    labels, sizes, _, _ = dc.expected(calls[:1], 600, dc.T, dc.U)
    assert set(labels.tolist()) == {0, 300} and (sizes == 300).all()
    labels, sizes, _, _ = dc.expected(calls, 600, dc.T, dc.U)
    assert not labels.any() and (sizes == 600).all()
    labels, sizes, _, _ = dc.expected(dc.dense(1200, k=8, block=500), 1200, dc.T, dc.U)
    assert sorted(set(labels.tolist())) == [0, 500, 1000] and sorted(set(sizes.tolist())) == [200, 500]
    labels, sizes, reasons, counts = dc.expected(dc.twins(100), 100, dc.T, dc.U)
    assert not labels.any() and (sizes == 100).all() and counts.tolist() == [99, 0, 0] and not reasons[0].any()
    labels, sizes, reasons, counts = dc.expected(dc.nothing(200), 200, dc.T, dc.U)
    assert labels.tolist() == list(range(200)) and (sizes == 1).all() and not counts.any() and not reasons[0].any()
    whole = dc.random_links(2000, 5, seed=11)
    for pieces in (3, 7):
        parts = dc.cut(whole[0], pieces)
        assert len(parts) == pieces and sum(c[1].shape[0] for c in parts) == 2000 and min(c[1].shape[0] for c in parts) > 0
        for a, b in zip(dc.expected(whole, 2000, dc.T, dc.U)[:2], dc.expected(parts, 2000, dc.T, dc.U)[:2]):
            assert np.array_equal(a, b)
    _, sizes, _, counts = dc.expected(whole, 2000, dc.T, dc.U)
    assert (counts > 0).all() and 1 in sizes and sizes.max() > 10


def test_edge_slots_known_answers():
    labels, sizes, (reasons,), counts = dc.expected(dc.edge_slots(), 300, dc.T, dc.U)
    assert reasons[0].tolist() == [0] * 8 and reasons[1].tolist() == [0] * 8
    assert reasons[2].tolist() == [0, 1, 0, 0, 1, 0, 1, 0]                         # 94 is not above 94, 95 is
    assert reasons[3].tolist() == [0, 2, 0, 0, 2, 0, 0, 2]                         # U is not above U, one ulp more is
    assert reasons[4].tolist() == [3, 2, 1, 0, 0, 0, 0, 2] and not reasons[5:].any()
    assert counts.tolist() == [2, 5, 5]                                            # exact: row 4 - 299 and row 7 - 50
    groups = {(2, 11, 14, 16), (3, 21, 24, 27), (4, 30, 31, 32, 299), (7, 50)}
    for group in groups:
        assert (labels[list(group)] == group[0]).all() and (sizes[list(group)] == len(group)).all()
    assert (sizes > 1).sum() == sum(len(g) for g in groups)


# ---- validate_duplicates, duplicate_frame, links_frame --------------------------------------------------------------------

@pytest.fixture
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the library was touched before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", refuse)


def test_validate_duplicates(no_library):
    assert prediction.validate_duplicates(94, 0.9) == (94, 0.9)
    lev, prob = prediction.validate_duplicates(np.int32(0), np.float32(0.5))
    assert type(lev) is int and lev == 0 and type(prob) is float and prob == 0.5
    assert prediction.validate_duplicates(100, 1) == (100, 1.0)
    assert prediction.validate_duplicates(50, -3.5) == (50, -3.5)


@pytest.mark.parametrize("lev, prob, message", [
    (101, 0.9, r"\[0, 100\]"), (-1, 0.9, r"\[0, 100\]"), (94.0, 0.9, "integer"), (True, 0.9, "integer"),
    ("94", 0.9, "integer"), ([94], 0.9, "integer"), (94, np.nan, "finite"), (94, np.inf, "finite"),
    (94, -np.inf, "finite"), (94, 1e300, "finite"), (94, "0.9", "finite number"), (94, True, "finite number"),
    (94, [0.9], "finite number"),
])
def test_validate_duplicates_refuses(no_library, lev, prob, message):
    with pytest.raises(ValueError, match=message):
        prediction.validate_duplicates(lev, prob)
    p = prediction.Prediction.__new__(prediction.Prediction)
    p.levenshtein_threshold, p.probability_threshold = 94, 0.9
    with pytest.raises(ValueError, match=message):
        p.duplicate_groups(lev, prob)
    p.levenshtein_threshold, p.probability_threshold = lev, prob              # None takes the instance's own value
    with pytest.raises(ValueError, match=message):
        p.duplicate_groups()


def test_duplicate_frame():
    ids = np.array([70, 10, 60, 20, 50, 30, 40, 0], dtype=np.int64)
    labels = np.array([0, 1, 1, 0, 4, 1, 6, 0], dtype=np.int32)
    sizes = np.array([3, 3, 3, 3, 1, 3, 1, 3], dtype=np.int32)
    frame = prediction.duplicate_frame(labels, sizes, ids)
    assert tuple(frame.columns) == prediction.DUPLICATE_COLUMNS == ("group_id", "group_size", "title_id", "row")
    assert frame["row"].tolist() == [0, 3, 7, 1, 2, 5]                            # by the group's lowest row, then by row
    assert frame["group_id"].tolist() == [70, 70, 70, 10, 10, 10]                 # the title id of the lowest row
    assert frame["group_size"].tolist() == [3] * 6 and frame["title_id"].tolist() == [70, 20, 0, 10, 60, 30]
    assert frame.dtypes.tolist() == [np.int64] * 4
    empty = prediction.duplicate_frame(np.arange(4), np.ones(4, dtype=np.int32), ids[:4])
    assert len(empty) == 0 and tuple(empty.columns) == prediction.DUPLICATE_COLUMNS
    assert empty.dtypes.tolist() == [np.int64] * 4
    # straight from the restatement
    labels, sizes = dc.components(8, [[5, 3], [7, 5], [2, 6]])
    assert prediction.duplicate_frame(labels, sizes, ids)["row"].tolist() == [2, 6, 3, 5, 7]


def test_links_frame():
    ids = np.arange(100, 112, dtype=np.int64)
    rows = np.array([[1, 7, 5], [0, 9, -1], [6, 6, 3]], dtype=np.int32)
    ratios = np.array([[95, 94, 100], [0, 100, 100], [96, 0, 0]], dtype=np.uint8)
    p = np.array([[0.95, 0.95, 1.0], [0.9, 1.0, 1.0], [np.nan, 0.91, 0.5]], dtype=np.float32)
    exact = np.array([8, -1, 7], dtype=np.int32)
    edges, reasons, _ = dc.links_of(rows, ratios, p, exact, 5, 9, 94, 0.9)
    frame = prediction.links_frame([(5, rows, ratios, p, exact, reasons)], ids, 9)
    assert tuple(frame.columns) == prediction.LINK_COLUMNS
    assert np.array_equal(frame[["row", "match_row"]].to_numpy(), edges)
    assert frame["stage"].tolist() == [1, 2, 3, 2, 3] and frame["levenshtein_ratio"].tolist() == [100, 95, 94, 96, 0]
    assert np.array_equal(frame["probability"].to_numpy(), np.array([np.nan, 0.95, 0.95, np.nan, 0.91], np.float32),
                          equal_nan=True)
    assert frame["title_id"].tolist() == [105, 105, 105, 107, 107] and frame["match_title_id"].tolist() == [108, 101, 107, 106, 106]
    assert [str(t) for t in frame.dtypes] == ["int64"] * 4 + ["uint8", "float32", "int8"]
    # two chunks follow each other; without the model the probability is NaN
    first = dc.links_of(rows[:2], ratios[:2], None, exact[:2], 5, 9, 94, 0.9)
    second = dc.links_of(rows[2:], ratios[2:], None, exact[2:], 7, 9, 94, 0.9)
    frame = prediction.links_frame([(5, rows[:2], ratios[:2], None, exact[:2], first[1]),
                                    (7, rows[2:], ratios[2:], None, exact[2:], second[1])], ids, 9)
    assert np.array_equal(frame[["row", "match_row"]].to_numpy(), np.concatenate((first[0], second[0])))
    assert frame["stage"].tolist() == [1, 2, 2] and frame["probability"].isna().all()
    empty = prediction.links_frame([], ids, 9)
    assert len(empty) == 0 and [str(t) for t in empty.dtypes] == ["int64"] * 4 + ["uint8", "float32", "int8"]


def test_link_columns_known_answers_and_links_frame_on_a_random_call():
    ids = np.arange(100, 112, dtype=np.int64)
    rows = np.array([[1, 7, 5], [0, 9, -1], [6, 6, 3]], dtype=np.int32)
    ratios = np.array([[95, 94, 100], [0, 100, 100], [96, 0, 0]], dtype=np.uint8)
    p = np.array([[0.95, 0.95, 1.0], [0.9, 1.0, 1.0], [np.nan, 0.91, 0.5]], dtype=np.float32)
    exact = np.array([8, -1, 7], dtype=np.int32)
    columns = dc.link_columns(rows, ratios, p, exact, 5, 9, 94, 0.9, ids)
    assert tuple(columns) == prediction.LINK_COLUMNS
    assert columns["row"].tolist() == [5, 5, 5, 7, 7] and columns["match_row"].tolist() == [8, 1, 7, 6, 6]
    assert columns["title_id"].tolist() == [105, 105, 105, 107, 107]
    assert columns["match_title_id"].tolist() == [108, 101, 107, 106, 106]
    assert columns["stage"].tolist() == [1, 2, 3, 2, 3] and columns["levenshtein_ratio"].tolist() == [100, 95, 94, 96, 0]
    assert np.array_equal(columns["probability"], np.array([np.nan, 0.95, 0.95, np.nan, 0.91], np.float32), equal_nan=True)
    assert [str(c.dtype) for c in columns.values()] == ["int64"] * 4 + ["uint8", "float32", "int8"]
    without = dc.link_columns(rows, ratios, None, None, 5, 9, 94, 0.9, ids)
    assert without["match_row"].tolist() == [1, 6] and without["stage"].tolist() == [2, 2]
    assert np.isnan(without["probability"]).all()
    # links_frame on 2,000 rows of 7 slots, cut into three chunks, against the restatement of the whole call
    (call,) = dc.random_links(2000, 7, seed=11)
    ids = np.arange(2000, dtype=np.int64) * 3 + 1
    chunks = [(q, r, l, pr, e, dc.links_of(r, l, pr, e, q, 2000, dc.T, dc.U)[1]) for q, r, l, pr, e in dc.cut(call, 3)]
    frame = prediction.links_frame(chunks, ids, 2000)
    columns = dc.link_columns(call[1], call[2], call[3], call[4], 0, 2000, dc.T, dc.U, ids)
    assert len(frame) > 2000 and set(frame["stage"].tolist()) == {1, 2, 3}
    for name in prediction.LINK_COLUMNS:
        assert frame[name].dtype == columns[name].dtype, name
        assert np.array_equal(frame[name].to_numpy(), columns[name], equal_nan=name == "probability"), name


# ---- the C ABI surface ----------------------------------------------------------------------------------------------

def test_header_declares_what_the_binding_calls():
    header = open(os.path.join(ROOT, "include", "doppel_amd.h")).read()

    def types_of(name):
        declaration = re.search(r"int %s\(([^;]*)\);" % name, header)
        assert declaration, f"{name} is not declared"
        arguments = [a.strip() for a in declaration.group(1).replace("\n", " ").split(",")]
        return [a.rsplit(" ", 1)[0] + ("*" if a.rsplit(" ", 1)[1].startswith("*") else "") for a in arguments]

    assert types_of("ds_duplicate_begin_device") == ["int32_t*", "int64_t", "int64_t*", "void*"]
    assert types_of("ds_duplicate_links_device") == [
        "const int32_t*", "const uint8_t*", "const float*", "const int32_t*", "int64_t", "int64_t", "int32_t", "int64_t",
        "int32_t", "float", "int32_t*", "uint8_t*", "int64_t*", "void*"]
    assert types_of("ds_duplicate_finish_device") == ["int32_t*", "int64_t", "int32_t*", "int32_t*", "void*"]
    assert re.search(r"int ds_duplicates_option\(const char \*name, int64_t value\);", header)
    assert {"ds_duplicate_begin_device", "ds_duplicate_links_device", "ds_duplicate_finish_device",
            "ds_duplicates_option"} <= set(_lib.EXPORTED_SYMBOLS)
    assert "ds_duplicates.hip" in _lib._SOURCES


@pytest.fixture(scope="module")
def library():
    """The library with the binding's argument types, loaded without asking for a device."""
    import doppel_speller_amd as ds
    handle = _lib._declare(ctypes.CDLL(ds.build_library()))
    return handle


def test_argument_errors_need_no_device(library):
    """Every bad argument is refused before the first HIP call: the pointers here are never dereferenced."""
    some = ctypes.c_void_p(0x1000)
    null = ctypes.c_void_p(0)
    good = [some, some, some, some, 0, 8, 5, 100, 94, 0.9, some, some, some, null]
    call = library.ds_duplicate_links_device
    for position in (0, 1, 10, 12):                                   # rows, ratios, parent, counts
        bad = list(good)
        bad[position] = null
        assert call(*bad) == -1 and b"null" in library.ds_last_error(), position
    for position, value, word in ((4, -1, b"negative"), (5, -1, b"negative"), (6, 0, b"positive"), (6, -2, b"positive"),
                                  (7, -1, b"n_truth"), (7, 1 << 31, b"n_truth"), (8, -1, b"[0, 100]"),
                                  (8, 101, b"[0, 100]"), (9, float("nan"), b"finite"), (9, float("inf"), b"finite"),
                                  (9, float("-inf"), b"finite"), (4, 93, b"not rows"), (5, 101, b"not rows"),
                                  (5, 1 << 62, b"too many")):
        bad = list(good)
        bad[position] = value
        assert call(*bad) == -1 and word in library.ds_last_error(), (position, value, library.ds_last_error())
    begin = library.ds_duplicate_begin_device
    assert begin(null, 10, some, null) == -1 and begin(some, 10, null, null) == -1
    assert b"null" in library.ds_last_error()
    assert begin(some, -1, some, null) == -1 and begin(some, 1 << 31, some, null) == -1
    finish = library.ds_duplicate_finish_device
    for position in (0, 2, 3):
        bad = [some, 10, some, some, null]
        bad[position] = null
        assert finish(*bad) == -1 and b"null" in library.ds_last_error(), position
    assert finish(some, -1, some, some, null) == -1 and finish(some, 1 << 31, some, some, null) == -1
    # nothing to do: no launch, no device needed
    empty = list(good)
    empty[5] = 0
    assert call(*empty) == 0
    empty = list(good)
    empty[4], empty[5], empty[7] = 0, 0, 0
    assert call(*empty) == 0 and finish(some, 0, some, some, null) == 0
    option = library.ds_duplicates_option
    assert option(b"max_blocks", -1) == -1 and option(b"max_blocks", (1 << 20) + 1) == -1
    assert option(b"no_such_option", 1) == -1 and option(None, 1) == -1
    assert option(b"max_blocks", 1) == 0 and option(b"max_blocks", 1 << 20) == 0 and option(b"max_blocks", 0) == 0


def test_package_exports():
    import doppel_speller_amd as ds
    assert ds.DUPLICATE_COLUMNS == prediction.DUPLICATE_COLUMNS and ds.LINK_COLUMNS == prediction.LINK_COLUMNS
    assert ds.validate_duplicates is prediction.validate_duplicates and ds.duplicate_frame is prediction.duplicate_frame
    assert callable(ds.Prediction.duplicate_groups) and "duplicate_groups" in ds.__doc__
    for name in ("enqueue_duplicate_links", "duplicate_reasons"):
        assert callable(getattr(ds.CandidatePipeline, name))
