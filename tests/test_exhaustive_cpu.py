"""Exhaustive matches without a GPU: the NumPy restatement of the rule (tests/exhaustive_cases.py) against a plain-Python
transcription with sorted(), the planted tables of the GPU tests against both, the grid caps those tests reach past against
the kernel's source, exhaustive_matches' argument checks, the frame it builds, and the C ABI surface."""
import os
import re

import numpy as np
import pytest

import exhaustive_cases as ec
from doppel_speller_amd import _lib, pipeline, prediction

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("kind", ec.KINDS)
@pytest.mark.parametrize("n_rows", [1, 3, 64, 65, 300])
def test_restatement_equals_the_sorted_transcription(n_rows, kind):
    probabilities = ec.make_probabilities(5, n_rows, kind, seed=n_rows, marks=(n_rows // 2, n_rows // 2 + 1))
    for n in (1, 5, 64):                # n = 64 above N = 1, 3: unfilled slots
        for row_first in (0, 1000):
            assert ec.as_lists(ec.best_rows(probabilities, n, row_first)) == \
                ec.best_rows_python(probabilities, n, row_first), (n, row_first)


def test_crafted_groups():
    probabilities = np.array([[.5, .5, .5, .5, .5, .5],       # all equal: the lowest rows
                              [.25, .75, .5, .75, .0, .75],   # equal bits at rows 1, 3, 5
                              [0., 0., 0., 0., 0., 0.],       # +0.0 everywhere: still the lowest rows, never "empty"
                              [.1, .2, .3, .4, .5, .6]], dtype=np.float32)
    row, probability = ec.best_rows(probabilities, 4)
    assert row.tolist() == [[0, 1, 2, 3], [1, 3, 5, 2], [0, 1, 2, 3], [5, 4, 3, 2]]
    assert probability[1].tolist() == [.75, .75, .75, .5] and probability[2].tolist() == [0.] * 4
    assert ec.best_rows(probabilities, 1)[0][:, 0].tolist() == [0, 1, 0, 5]
    # N < n: the six rows in order, then (-1, the quiet NaN)
    row, probability = ec.best_rows(probabilities, 64)
    assert row[3, :6].tolist() == [5, 4, 3, 2, 1, 0] and (row[:, 6:] == -1).all()
    assert (probability[:, 6:].view(np.uint32) == 0x7fc00000).all()
    assert ec.as_lists((row, probability)) == ec.best_rows_python(probabilities, 64)
    # equal bits at far-apart rows of a long table
    far = np.zeros((1, 100000), dtype=np.float32)
    far[0, [99999, 7, 65536]] = 0.5
    assert ec.best_rows(far, 5)[0].tolist() == [[7, 65536, 99999, 0, 1]]
    assert ec.as_lists(ec.best_rows(far, 5)) == ec.best_rows_python(far, 5)
    # the keys of the running list: never 0 for a row, 0 for an empty slot, descending
    keys = ec.best_keys(probabilities, 8, row_first=10)
    assert keys.dtype == np.uint64 and (keys[:, :6] != 0).all() and (keys[:, 6:] == 0).all()
    assert (np.diff(keys[:, :6].astype(object), axis=1) < 0).all()
    assert keys[2, 0] == 0xffffffff - 10 and keys[3, 0] == (int(np.float32(.6).view(np.uint32)) << 32) | (0xffffffff - 15)


def test_split_covers_the_rows_with_a_ragged_last_call():
    for n_rows in (1, 63, 64, 65, 8193):
        for calls in (1, 2, 7):
            ranges = ec.split(n_rows, calls)
            assert ranges[0][0] == 0 and ranges[-1][1] == n_rows and len(ranges) <= calls
            assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
            if calls > 1 and n_rows > calls:
                assert len(ranges) > 1 and ranges[-1][1] - ranges[-1][0] < ranges[0][1] - ranges[0][0]


@pytest.mark.parametrize("n", [1, 5, 64])
def test_planted_winners_are_what_the_rule_returns(n):
    """make_planted's closed form against best_rows and best_rows_python: default rows, the caller's rows, two calls."""
    n_rows = 20000
    chosen = [0, n_rows - 1] + [4095 + 211 * j for j in range(n - 2)] if n > 1 else [n_rows - 1]
    for rows in (None, chosen):
        probabilities, winners = ec.make_planted(n_rows, n, seed=n, rows=rows)
        assert probabilities.shape == (1, n_rows) and probabilities.dtype == np.float32
        assert winners.shape == (1, n) and winners.dtype == np.int32
        spread = [0] if n == 1 else [s * (n_rows - 1) // (n - 1) for s in range(n)]     # the documented default
        assert sorted(winners[0].tolist()) == sorted(rows if rows else spread)
        assert rows or n == 1 or {0, n_rows - 1} <= set(winners[0].tolist())
        planted = probabilities[0, winners[0]]
        assert (planted >= 0.5).all() and (np.delete(probabilities[0], winners[0]) < 0.5).all()
        assert (np.diff(planted) <= 0).all()
        best = ec.best_rows(probabilities, n)
        assert np.array_equal(best[0], winners) and np.array_equal(best[1][0], planted)
        assert ec.as_lists(best) == ec.best_rows_python(probabilities, n)
        assert np.array_equal(ec.keys_of(best), ec.best_keys(probabilities, n))
        # the pairs: the same bits at two rows, the lower row first and right in front of the other
        units = ec.planted_units(winners[0])
        pairs = [unit for unit in units if len(unit) == 2]
        assert len(pairs) == (n // 2 + 1) // 2 and sum(len(unit) for unit in units) == n
        at = {row: slot for slot, row in enumerate(winners[0].tolist())}
        for low, high in pairs:
            assert low < high and at[high] == at[low] + 1 and probabilities[0, low] == probabilities[0, high]
        assert len(set(planted.tolist())) == len(units)
        # with the table moved by row_first the winners move with it
        assert np.array_equal(ec.best_rows(probabilities, n, 1000)[0], winners + 1000)


def test_the_caps_the_gpu_tests_reach_past_are_the_sources():
    """The shapes of test_gpu_exhaustive_kernel.py and test_gpu_exhaustive.py are chosen from the grid caps and the fold
    arithmetic of csrc/ds_exhaustive.hip.  Whoever moves one of them learns here that those tests no longer reach past it."""
    import test_gpu_exhaustive as stage_tests
    import test_gpu_exhaustive_kernel as kernel_tests
    source = open(os.path.join(ROOT, "doppel-speller_amd", "csrc", "ds_exhaustive.hip")).read()

    def constant(name):
        found = re.search(r"constexpr (?:int|int64_t) %s = ([^;]+);" % name, source)
        assert found, name
        return found.group(1).strip()

    assert int(constant("kFoldThreads")) == kernel_tests.FOLD_THREADS
    assert int(constant("kFoldKeysPerThread")) == kernel_tests.KEYS_PER_THREAD
    assert constant("kSliceKeys") == "kFoldThreads * kFoldKeysPerThread"
    assert kernel_tests.SLICE_KEYS == kernel_tests.FOLD_THREADS * kernel_tests.KEYS_PER_THREAD == 4096
    assert int(constant("kExhaustiveMaxN")) == kernel_tests.MAX_N == pipeline.EXHAUSTIVE_MAX_N
    assert constant("kTilePairsMax") == "int64_t(1) << 24" and kernel_tests.TILE_PAIRS_MAX == 1 << 24

    # the three capped grids, each in the function that launches the kernel
    def grid_cap(after, kernel):
        body = source[source.index(after):]
        body = body[:body.index(kernel)]
        caps = re.findall(r"std::min<int64_t>\(([^;]*), 256 \* (\d+)\)\);", body)
        assert len(caps) == 1, (after, caps)
        return caps[0][0], 256 * int(caps[0][1])

    assert len(re.findall(r"std::min<int64_t>\([^;]*, 256 \* \d+\)", source)) == 3
    assert grid_cap("static int fold(", "DS_LAUNCH(ds_exhaustive_select_kernel") == \
        ("args.n_blocks", kernel_tests.SELECT_BLOCKS_MAX)
    assert grid_cap("int ds_exhaustive_finish_device(", "DS_LAUNCH(ds::ds_exhaustive_finish_kernel") == \
        ("(n_slots + 255) / 256", kernel_tests.FINISH_SLOTS_MAX // 256)
    assert grid_cap("int ds_exhaustive_rank_device(", "DS_LAUNCH(ds::ds_exhaustive_pairs_kernel") == \
        ("(here + 255) / 256", stage_tests.PAIRS_KERNEL_PAIRS_MAX // 256)
    assert (kernel_tests.SELECT_BLOCKS_MAX, kernel_tests.FINISH_SLOTS_MAX, stage_tests.PAIRS_KERNEL_PAIRS_MAX) == \
        (16384, 1048576, 1048576)
    # the kernels stride by what they were launched with: a workgroup of the pairs and finish kernels is 256 threads
    assert "i += gridDim.x * 256u)" in source and "i += static_cast<int64_t>(gridDim.x) * 256)" in source
    assert "block += gridDim.x)" in source

    # the fold arithmetic behind the level tests: slices per level of one query
    top = kernel_tests.TILE_PAIRS_MAX
    assert ec.fold_levels(top - 64, 64) == [4096, 64, 1]
    assert ec.fold_levels(top - 63, 64) == ec.fold_levels(top, 64) == [4097, 65, 2, 1]
    assert ec.fold_levels(300000, 64) == [74, 2, 1] and ec.fold_levels(300000, 5) == [74, 1]
    assert ec.fold_levels(100, 64) == [1] and ec.fold_levels(4100, 5) == [2, 1] and ec.fold_levels(4091, 5) == [1]


@pytest.fixture
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the library was touched before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", refuse)


def _unbuilt(n_truth):
    p = prediction.Prediction.__new__(prediction.Prediction)
    p.top_n = 10
    p.truth_titles = ["t"] * n_truth
    return p


@pytest.mark.parametrize("n", [0, -1, True, False, 2.0, "3", None, 65, np.int64(0)])
def test_bad_n_is_refused_before_any_device_work(no_library, n):
    with pytest.raises(ValueError, match="^n "):
        _unbuilt(1000).exhaustive_matches(["a title"], n=n)
    with pytest.raises(ValueError, match="^n "):
        prediction.validate_exhaustive(n, 1000)


def test_n_is_checked_against_64_and_the_truth_titles(no_library):
    assert prediction.validate_exhaustive(1, 1) == 1 and prediction.validate_exhaustive(np.int32(64), 64) == 64
    assert prediction.validate_exhaustive(64, 10 ** 6) == 64 and pipeline.EXHAUSTIVE_MAX_N == 64
    with pytest.raises(ValueError, match="48 truth titles"):
        prediction.validate_exhaustive(49, 48)
    with pytest.raises(ValueError, match="48 truth titles"):
        _unbuilt(48).exhaustive_matches(["a title"], n=49)
    with pytest.raises(ValueError, match="test indexes"):
        _unbuilt(48).exhaustive_matches(["a", "b"], n=3, test_index=[1, 1])


def test_jaccard_positions():
    top_rows = np.array([[5, 9, 2, 7], [1, 1, 3, 0], [8, 6, 4, 2]], dtype=np.int32)
    rows = np.array([[5, 7, 3], [1, 0, -1], [-1, -1, -1]], dtype=np.int32)
    positions = prediction.jaccard_positions(rows, top_rows)
    # position 0, position top_n - 1, absent; the first of a repeated row; an unfilled slot is never "found"
    assert positions.dtype == np.int32 and positions.tolist() == [[0, 3, -1], [0, 3, -1], [-1, -1, -1]]
    assert prediction.jaccard_positions(rows[:0], top_rows[:0]).shape == (0, 3)
    failed = np.full((1, 4), -1, dtype=np.int32)          # a failed top-k leaves -1 rows: they match nothing
    assert prediction.jaccard_positions(np.array([[2, -1]], dtype=np.int32), failed).tolist() == [[-1, -1]]


def test_exhaustive_frame():
    ids = np.array([100, 101, 102, 103], dtype=np.int64)
    rows = np.array([[2, 0, 3], [1, -1, -1], [3, 1, 0]], dtype=np.int32)
    probabilities = np.array([[.75, .5, .5], [.25, np.nan, np.nan], [.9, .9, .1]], dtype=np.float32)
    top_rows = np.array([[2, 1], [0, 2], [0, 3]], dtype=np.int32)
    frame = prediction.exhaustive_frame([7, 5, 3], rows, probabilities, top_rows, ids)
    assert tuple(frame.columns) == prediction.EXHAUSTIVE_COLUMNS == (
        "test_index", "rank", "title_id", "match_row", "probability", "jaccard_position")
    assert frame["test_index"].tolist() == [3, 3, 3, 5, 7, 7, 7] and frame["rank"].tolist() == [1, 2, 3, 1, 1, 2, 3]
    assert frame["match_row"].tolist() == [3, 1, 0, 1, 2, 0, 3]
    assert frame["title_id"].tolist() == [103, 101, 100, 101, 102, 100, 103]
    assert frame["jaccard_position"].tolist() == [1, -1, 0, -1, 0, -1, -1]
    assert frame["probability"].tolist() == [np.float32(v) for v in (.9, .9, .1, .25, .75, .5, .5)]
    assert [str(t) for t in frame.dtypes] == ["int64", "int64", "int64", "int64", "float32", "int32"]
    empty = prediction.exhaustive_frame(np.zeros(0, np.int64), rows[:0], probabilities[:0], top_rows[:0], ids)
    assert tuple(empty.columns) == prediction.EXHAUSTIVE_COLUMNS and len(empty) == 0
    assert empty.dtypes.tolist() == frame.dtypes.tolist()


def test_header_declares_what_the_binding_calls():
    header = open(os.path.join(ROOT, "include", "doppel_amd.h")).read()

    def types(name):
        declaration = re.search(r"int %s\(([^;]*)\);" % name, header)
        assert declaration, name + " is not declared"
        text = re.sub(r"/\*.*?\*/", "", declaration.group(1).replace("\n", " "))
        arguments = [a.strip() for a in text.split(",")]
        return [a.rsplit(" ", 1)[0] + ("*" if a.rsplit(" ", 1)[1].startswith("*") else "") for a in arguments]

    assert types("ds_exhaustive_fold_device") == ["const float*", "int64_t", "int64_t", "int64_t", "int32_t", "uint64_t*",
                                                  "void*"]
    assert types("ds_exhaustive_finish_device") == ["const uint64_t*", "int64_t", "int32_t", "int32_t*", "float*", "void*"]
    assert types("ds_exhaustive_rank_device") == ["ds_titles*", "ds_titles*", "ds_forest*", "int64_t", "int64_t", "int32_t",
                                                  "uint8_t", "uint32_t", "int32_t*", "float*", "void*"]
    assert re.search(r"int ds_exhaustive_option\(const char \*name, int64_t value\);", header)
    assert {"ds_exhaustive_fold_device", "ds_exhaustive_finish_device", "ds_exhaustive_rank_device",
            "ds_exhaustive_option"} <= set(_lib.EXPORTED_SYMBOLS)
    assert "ds_exhaustive.hip" in _lib._SOURCES


def test_package_exports():
    import doppel_speller_amd as ds
    assert ds.EXHAUSTIVE_COLUMNS == prediction.EXHAUSTIVE_COLUMNS and ds.validate_exhaustive is prediction.validate_exhaustive
    assert callable(ds.Prediction.exhaustive_matches)
    assert callable(ds.CandidatePipeline.enqueue_exhaustive) and callable(ds.CandidatePipeline.exhaustive)
    assert "exhaustive_matches" in ds.__doc__
    import inspect
    assert inspect.signature(ds.Prediction.closest_search_single_title).parameters["exhaustive"].default is False
