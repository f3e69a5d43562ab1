"""ds_exhaustive_fold_device and ds_exhaustive_finish_device through the C ABI, on crafted probabilities, against the NumPy
restatement of the rule (tests/exhaustive_cases.py), bit for bit: every shape folded in 1, 2 and 7 calls, ties across slice
and call boundaries, fewer rows than slots, the level structure of a long tile, the argument errors; query counts past the
select and finish kernels' grid caps, and a tile of 2^24 rows that takes every level the fold can reach below 8 GB of
probabilities (a fifth level needs a tile of nearly 2^31 rows and is left out)."""
import numpy as np
import pytest

import exhaustive_cases as ec
from doppel_speller_amd import _lib

pytestmark = pytest.mark.gpu

# What the shapes below are chosen from (tests/test_exhaustive_cpu.py holds them against csrc/ds_exhaustive.hip)
FOLD_THREADS, KEYS_PER_THREAD = 256, 16
SLICE_KEYS = 4096              # keys one workgroup of ds_exhaustive_select_kernel holds (kSliceKeys)
MAX_N = 64
SELECT_BLOCKS_MAX = 256 * 64   # workgroups of ds_exhaustive_select_kernel at most: the rest by its block loop
FINISH_SLOTS_MAX = 256 * 16 * 256   # slots ds_exhaustive_finish_kernel's grid covers: the rest by its stride
TILE_PAIRS_MAX = 1 << 24       # rows of one query ds_exhaustive_rank_device asks the fold for at most


def _fold(probabilities, n, calls, row_first=0, ranges=None):
    """The running keys and the finished slots after folding the table in `calls` calls (or in the calls of `ranges`)."""
    n_queries, n_rows = probabilities.shape
    running = _lib.DeviceArray.from_host(np.zeros((n_queries, n), dtype=np.uint64))
    for first, last in ranges or ec.split(n_rows, calls):
        tile = _lib.DeviceArray.from_host(np.ascontiguousarray(probabilities[:, first:last]))
        _lib.check(_lib.lib().ds_exhaustive_fold_device(tile.ptr, n_queries, last - first, row_first + first, n,
                                                        running.ptr, _lib.pointer(None)), "ds_exhaustive_fold_device")
    outputs = [_lib.DeviceArray((n_queries * n,), dtype) for dtype in (np.int32, np.float32)]
    for out in outputs:                 # a slot the kernel leaves out shows as 0x55 bytes
        _lib.check(_lib.lib().ds_memset(out.ptr, 0x55, out.nbytes, 0), "ds_memset")
    _lib.check(_lib.lib().ds_exhaustive_finish_device(running.ptr, n_queries, n, *(a.ptr for a in outputs),
                                                      _lib.pointer(None)), "ds_exhaustive_finish_device")
    _lib.check(_lib.lib().ds_stream_sync(_lib.pointer(None), 0), "sync")
    return running.to_host(), tuple(a.to_host().reshape(n_queries, n) for a in outputs)


def _marks(n_rows, calls):
    """Rows either side of every call boundary and of every slice boundary inside a call."""
    marks = []
    for first, last in ec.split(n_rows, calls):
        marks += [first - 1, first] + [first + at for at in range(SLICE_KEYS - 1, last - first, SLICE_KEYS)] + \
                 [first + at for at in range(SLICE_KEYS, last - first, SLICE_KEYS)]
    return tuple(marks)


@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 8193])
@pytest.mark.parametrize("n", [1, 5, 64])
@pytest.mark.parametrize("n_queries", [1, 3])
def test_every_shape_in_one_two_and_seven_calls(n_queries, n, n_rows):
    """n = 64 above 1 and 63 rows leaves unfilled slots; "equal" must give the lowest rows; "straddle" puts the one
    maximum either side of every slice and call boundary."""
    for kind in ec.KINDS:
        for calls in (1, 2, 7):
            probabilities = ec.make_probabilities(n_queries, n_rows, kind, seed=n_rows + n, marks=_marks(n_rows, calls))
            keys, slots = _fold(probabilities, n, calls, row_first=0)
            what = (kind, calls)
            assert np.array_equal(keys, ec.best_keys(probabilities, n)), what
            assert ec.same_best(slots, ec.best_rows(probabilities, n)), what
            if kind == "equal":
                assert (slots[0][:, :min(n, n_rows)] == np.arange(min(n, n_rows))).all(), what


def test_rows_that_do_not_start_at_zero_and_a_fold_of_no_rows():
    probabilities = ec.make_probabilities(3, 200, "few", seed=9)
    keys, slots = _fold(probabilities, 5, 2, row_first=2 ** 31 - 200)          # the last rows a key can hold
    assert ec.same_best(slots, ec.best_rows(probabilities, 5, 2 ** 31 - 200))
    assert np.array_equal(keys, ec.best_keys(probabilities, 5, 2 ** 31 - 200))
    running = _lib.DeviceArray.from_host(keys)
    tile = _lib.DeviceArray((1,), np.float32)
    fold = _lib.lib().ds_exhaustive_fold_device
    assert fold(tile.ptr, 3, 0, 0, 5, running.ptr, _lib.pointer(None)) == 0        # no rows: nothing changes
    assert fold(tile.ptr, 0, 10, 0, 5, running.ptr, _lib.pointer(None)) == 0       # no queries
    _lib.check(_lib.lib().ds_stream_sync(_lib.pointer(None), 0), "sync")
    assert np.array_equal(running.to_host(), keys)


@pytest.mark.parametrize("n", [5, 64])
def test_a_tile_long_enough_for_every_level(n):
    """300,000 rows of one query: 74 slices at level 0; at n = 64 their 4,736 keys take two slices at level 1 and a level
    2, at n = 5 level 1 is the last.  Ties everywhere ("few"), and the same table in two calls."""
    probabilities = ec.make_probabilities(1, 300000, "few", seed=n)
    probabilities[0, [299999, 150000, 4095, 4096]] = 0.875
    expected = ec.best_rows(probabilities, n)
    assert expected[0][0, :4].tolist() == [4095, 4096, 150000, 299999]
    for calls in (1, 2):
        keys, slots = _fold(probabilities, n, calls)
        assert ec.same_best(slots, expected), calls
        assert np.array_equal(keys, ec.best_keys(probabilities, n)), calls


@pytest.mark.parametrize("n, n_rows", [(1, 100), (5, 100), (64, 100), (64, 40)])
def test_query_counts_past_the_select_grid_one_slice_per_query(n, n_rows):
    """16,384 + 5 queries of one slice each: the last five workgroups take a second block, with the LDS words of their first
    one.  At n = 64 the 1,048,896 slots are past the finish kernel's grid as well.  40 rows at n = 64: every block runs dry
    after 40 (or 21 and 40) rounds, breaks out and zero-fills, on the second trip too."""
    n_queries = SELECT_BLOCKS_MAX + 5
    assert ec.fold_levels(n_rows, n) == [1]
    if n == 64:
        assert n_queries * n == 1048896 > FINISH_SLOTS_MAX
    for kind in ("few", "equal", "straddle"):
        for calls in (1, 2):
            probabilities = ec.make_probabilities(n_queries, n_rows, kind, seed=n_rows + n, marks=_marks(n_rows, calls))
            expected = ec.best_rows(probabilities, n)
            keys, slots = _fold(probabilities, n, calls)
            what = (kind, calls)
            assert np.array_equal(keys, ec.keys_of(expected)), what
            assert ec.same_best(slots, expected), what
            if n_rows < n:
                assert (slots[0][:, n_rows:] == -1).all() and (keys[:, n_rows:] == 0).all() and (keys[:, :n_rows] != 0).all()


@pytest.mark.parametrize("kind", ["few", "straddle"])
def test_query_counts_past_the_select_grid_two_slices_per_query(kind):
    """8,200 queries x 4,100 rows, n = 5: 4,105 keys are two slices per query, so level 0 is 16,400 blocks on 16,384
    workgroups and level 1 is 8,200.  "straddle" puts the maximum either side of row 4,095 / 4,096 and of the boundary of
    the two calls (2,051, no multiple of 4,096).  Most of the time is NumPy's: 33.6M values made and sorted on the host."""
    n_queries, n_rows, n, chunk = 8200, 4100, 5, 1025
    assert ec.fold_levels(n_rows, n) == [2, 1] and n_queries * 2 == 16400 > SELECT_BLOCKS_MAX
    assert ec.split(n_rows, 2) == [(0, 2051), (2051, 4100)]
    marks = _marks(n_rows, 1) + _marks(n_rows, 2)
    assert {4095, 4096, 2050, 2051} <= set(marks)
    probabilities = np.concatenate([ec.make_probabilities(chunk, n_rows, kind, seed=q, marks=marks)
                                    for q in range(0, n_queries, chunk)])
    assert probabilities.shape == (n_queries, n_rows)
    parts = [ec.best_rows(probabilities[q:q + chunk], n) for q in range(0, n_queries, chunk)]    # 34 MB of keys at a time
    expected = tuple(np.concatenate([part[i] for part in parts]) for i in (0, 1))
    if kind == "straddle":
        assert (expected[0] == [0, 2050, 2051, 4095, 4096]).all()
    for calls in (1, 2):
        keys, slots = _fold(probabilities, n, calls)
        assert ec.same_best(slots, expected), calls
        assert np.array_equal(keys, ec.keys_of(expected)), calls


def _planted_rows(n_rows, first_call=()):
    """64 rows for make_planted in a table folded as `first_call` rows of a small first call (none: one call) and one tile
    of the rest: the first call's rows; in the tile, key 0, the last key, the keys either side of 2^24 - 64, and keys
    j * 2^18 + 61 j + 7 (j = 1 ...: a level-1 slice each when n = 64, a different place in its level-0 slice each)."""
    base = max(first_call) + 1 if first_call else 0
    rows = list(first_call) + [base, n_rows - 1] + \
        [base + key for key in (TILE_PAIRS_MAX - 65, TILE_PAIRS_MAX - 64) if base + key < n_rows - 1]
    rows += [base + (j << 18) + 61 * j + 7 for j in range(1, MAX_N - len(rows) + 1)]
    assert len(set(rows)) == len(rows) == MAX_N and max(rows) == n_rows - 1
    return rows


@pytest.mark.parametrize("n_rows, first_call, levels", [
    (TILE_PAIRS_MAX - 64, (), [4096, 64, 1]),           # every slice of every level exactly full
    (TILE_PAIRS_MAX, (), [4097, 65, 2, 1]),             # level-0 slice 4,096 holds the (empty) running list alone
    (100 + TILE_PAIRS_MAX, (0, 57, 99), [4097, 65, 2, 1])])   # ... and now three keys that belong among the 64
def test_every_level_of_the_fold_with_planted_winners(n_rows, first_call, levels):
    """One query, n = 64, a tile of up to 2^24 rows (what ds_exhaustive_rank_device asks for at most): three levels, and
    four, where level 2 has two slices and writes the first partial buffer while it reads the second.  The 64 winners are
    planted (ec.make_planted) at keys j * 2^18 + 61 j + 7, a level-1 slice each, but for the slots spent on the first and
    last rows, the keys either side of 2^24 - 64 and the first call's rows: 64, 62 and 59 of the level-1 slices of the
    three cases hold a winner.  Equal values come in pairs whose rows lie 2^23 apart.  In the single call of 2^24 rows
    level-0 slice 4,096, level-1 slice 64 and level-2 slice 1 hold the empty running list and pass on nothing.  In the
    last case rows 0 .. 99 are folded first, so the running list holds three winners when the tile of 2^24 rows comes:
    they travel alone through those three slices.  Most of the time is NumPy's: the sort of 16.7M keys behind best_rows."""
    tile_first = max(first_call) + 1 if first_call else 0
    assert ec.fold_levels(n_rows - tile_first, MAX_N) == levels and n_rows - tile_first <= TILE_PAIRS_MAX
    rows = _planted_rows(n_rows, first_call)
    assert {0, n_rows - 1, tile_first + TILE_PAIRS_MAX - 65} <= set(rows)
    assert len({(row - tile_first) >> 18 for row in rows if row >= tile_first}) == MAX_N - (0 if n_rows < TILE_PAIRS_MAX
                                                                                          else 5 if first_call else 2)
    assert all(len(unit) == 1 or unit[1] - unit[0] >= 1 << 18 for unit in ec.planted_units(rows))
    assert sum(len(unit) == 2 for unit in ec.planted_units(rows)) == 16
    probabilities, winners = ec.make_planted(n_rows, MAX_N, seed=len(levels), rows=rows)
    expected = ec.best_rows(probabilities, MAX_N)
    assert np.array_equal(expected[0], winners)
    ranges = [(0, tile_first), (tile_first, n_rows)] if first_call else None
    keys, slots = _fold(probabilities, MAX_N, 1, ranges=ranges)
    assert np.array_equal(slots[0], winners)
    assert ec.same_best(slots, expected)
    assert np.array_equal(keys, ec.keys_of(expected))


def test_argument_errors():
    probabilities = ec.make_probabilities(2, 100, "random", seed=1)
    tile = _lib.DeviceArray.from_host(probabilities)
    before = np.full((2, 5), 7, dtype=np.uint64)
    running = _lib.DeviceArray.from_host(before)
    fold, finish = _lib.lib().ds_exhaustive_fold_device, _lib.lib().ds_exhaustive_finish_device
    good = [tile.ptr, 2, 100, 0, 5, running.ptr, _lib.pointer(None)]
    for position, value in ((0, _lib.pointer(None)), (5, _lib.pointer(None)), (4, 0), (4, 65), (4, -1), (1, -1), (2, -1),
                            (3, -1), (3, 2 ** 31)):
        bad = list(good)
        bad[position] = value
        assert fold(*bad) == -1, (position, value)
        assert _lib.lib().ds_last_error()
    outputs = [_lib.DeviceArray.from_host(np.full(10, 0x55555555, dtype=np.int32)),
               _lib.DeviceArray.from_host(np.full(10, 0x55555555, dtype=np.int32).view(np.float32))]
    good_finish = [running.ptr, 2, 5, outputs[0].ptr, outputs[1].ptr, _lib.pointer(None)]
    for position, value in ((0, _lib.pointer(None)), (3, _lib.pointer(None)), (4, _lib.pointer(None)), (2, 0), (2, 65),
                            (1, -1)):
        bad = list(good_finish)
        bad[position] = value
        assert finish(*bad) == -1, (position, value)
    _lib.check(_lib.lib().ds_stream_sync(_lib.pointer(None), 0), "sync")
    # nothing was launched: the running list and the outputs are as they were
    assert np.array_equal(running.to_host(), before)
    assert (outputs[0].to_host() == 0x55555555).all() and (outputs[1].to_host().view(np.int32) == 0x55555555).all()
    option = _lib.lib().ds_exhaustive_option
    assert option(b"tile_pairs", -1) == -1 and option(b"tile_pairs", 2 ** 24 + 1) == -1
    assert option(b"no_such_option", 1) == -1 and option(None, 1) == -1
    assert option(b"tile_pairs", 0) == 0
    rank = _lib.lib().ds_exhaustive_rank_device
    assert rank(None, None, None, 0, 1, 5, 0, 1, outputs[0].ptr, outputs[1].ptr, _lib.pointer(None)) == -1
