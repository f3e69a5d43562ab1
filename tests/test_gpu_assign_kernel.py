"""ds_assign_edges_device and ds_assign_solve_device through the C ABI on the ranked slots of tests/assignment_cases.py -- no
model, no index -- against the restatement there, bit for bit: the keys, the three outputs per title and the four counts
that are a function of the input.  Proposals and rounds are diagnostics: bounded, never pinned."""
import ctypes

import numpy as np
import pytest

import assignment_cases as ac

pytestmark = pytest.mark.gpu

SENTINEL = 0x5a


def device_of(array):
    from doppel_speller_amd import _lib
    return _lib.DeviceArray.from_host(array) if array.size else _lib.DeviceArray((1,), array.dtype)


def run(case, at=(), solve=True):
    """The case's slots fed as chunks cut at `at`, then one solve -> (keys, rows, Result with all six counts)."""
    from doppel_speller_amd import _lib
    lib = _lib.lib()
    stream = ctypes.c_void_p(0)
    count, n = case.row.shape
    make = lambda shape, dtype: _lib.DeviceArray(shape, dtype)
    keys, rows = make((max(count, 1), n), np.uint64), make((max(count, 1), n), np.int32)
    held, standing = make((max(case.n_truth, 1),), np.uint64), make((max(count, 1),), np.int32)
    outputs = [make((max(count, 1),), np.int32) for _ in range(3)]
    counts = _lib.DeviceArray.from_host(np.full(6, -77, dtype=np.int64))
    for buffer in [keys, rows, held, standing] + outputs:                    # the stage writes or zeroes all of it
        _lib.check(lib.ds_memset(buffer.ptr, SENTINEL, buffer.nbytes, 0), "ds_memset")
    for q_first, *chunk in ac.cut(case, at):
        device = [device_of(np.ascontiguousarray(a)) for a in chunk]
        _lib.check(lib.ds_assign_edges_device(*(a.ptr for a in device), q_first, chunk[0].shape[0], count, n, case.n_truth,
                                              float(case.threshold), keys.ptr, rows.ptr, stream), "ds_assign_edges_device")
        _lib.check(lib.ds_stream_sync(None, 0), "sync")                      # the chunk's buffers go away here
    if not solve:
        return keys.to_host()[:count], rows.to_host()[:count], None
    _lib.check(lib.ds_assign_solve_device(rows.ptr, keys.ptr, count, n, case.n_truth, held.ptr, standing.ptr,
                                          *(a.ptr for a in outputs), counts.ptr, stream), "ds_assign_solve_device")
    # the solve has synchronised: what follows are plain copies
    result = ac.Result(*(a.to_host()[:count] for a in outputs), counts.to_host())
    if count and case.n_truth:
        now = held.to_host()
        matched = result.match_row >= 0
        mine = keys.to_host()[:count][np.nonzero(matched)[0], result.match_slot[matched]]
        assert np.array_equal(now[result.match_row[matched]], mine), "a title does not hold the row it was given"
        assert (now != 0).sum() == matched.sum()
    return keys.to_host()[:count], rows.to_host()[:count], result


def check(case, what, at=(), expected=None):
    want_keys = ac.keys_of(case)
    want = ac.deferred_acceptance(case.row, want_keys, case.n_truth) if expected is None else expected
    keys, rows, got = run(case, at)
    assert keys.dtype == np.uint64 and np.array_equal(keys, want_keys), (what, "keys", np.argwhere(keys != want_keys)[:5])
    assert np.array_equal(rows, case.row), (what, "rows")
    for name in ("match_row", "match_slot", "first_row"):
        mine, theirs = getattr(got, name), getattr(want, name)
        wrong = np.nonzero(mine != theirs)[0]
        assert mine.dtype == np.int32 and wrong.shape[0] == 0, (what, name, wrong.shape[0], wrong[:5], mine[wrong][:5],
                                                                theirs[wrong][:5])
    assert got.counts[:4].tolist() == want.counts.tolist(), (what, "counts", got.counts, want.counts)
    edges, matched = int(want.counts[0]), int(want.counts[1])
    assert matched <= got.counts[4] <= max(edges, 0), (what, "proposals", got.counts)
    # the first round moves every title; every later one has a title that a raise of the round before displaced
    assert (1 if case.row.shape[0] else 0) <= got.counts[5] <= got.counts[4] + 1, (what, "rounds", got.counts)
    return got


@pytest.fixture
def option():
    """Sets options of the stage for a test and puts the defaults back."""
    from doppel_speller_amd import _lib

    def choose(name, value):
        _lib.check(_lib.lib().ds_assign_option(name.encode(), value), "ds_assign_option")
    yield choose
    choose("max_blocks", 0)
    choose("rounds_per_sync", 8)


@pytest.fixture(scope="module")
def random_ties():
    case = ac.random_ties()
    return case, ac.expected(case)


def test_no_contention():
    got = check(ac.no_contention(1000, 3), "no contention")
    assert (got.match_slot == 0).all() and got.counts.tolist() == [3000, 1000, 0, 0, 1000, 1]
    assert np.array_equal(got.match_row, np.arange(1000) * 3) and np.array_equal(got.first_row, got.match_row)


def test_the_case_one_round_of_best_claimants_gets_wrong():
    got = check(ac.best_claimant(), "best claimant")
    assert got.match_row.tolist() == [0, -1, 1] and got.match_slot.tolist() == [1, -1, 0]
    assert got.first_row.tolist() == [1, 0, 1] and got.counts[:4].tolist() == [4, 2, 2, 1]


def test_a_chain_of_300_displacements():
    got = check(ac.chain(300), "chain")
    assert got.match_slot.tolist() == [0] + [1] * 300 and got.match_row.tolist() == list(range(301))
    assert got.counts[2] == 300 and got.counts[3] == 0
    assert got.counts[5] >= 2
    print("chain of 300: rounds", int(got.counts[5]), "proposals", int(got.counts[4]))


def test_classes_and_ties_at_one_row():
    got = check(ac.classes(), "classes")
    assert np.nonzero(got.match_row >= 0)[0].tolist() == list(ac.CLASS_WINNERS)
    assert got.counts[:4].tolist() == [13, 6, 7, 7]


def test_which_slots_are_edges():
    case, slots = ac.eligibility()
    assert check(case, "eligibility").match_slot.tolist() == slots.tolist()
    case, slots = ac.negative_threshold()
    assert check(case, "negative threshold").match_slot.tolist() == slots.tolist()
    got = check(ac.repeated_rows(), "repeated rows")
    assert got.match_row.tolist() == [1, 0] and got.match_slot.tolist() == [3, 0] and got.counts[0] == 3


def test_unordered_slots_follow_slot_order_not_score():
    case = ac.unordered()
    keys = ac.keys_of(case)
    got = check(case, "unordered")
    sorted_loop = ac.greedy(case.row, keys, case.n_truth)
    assert got.match_row[:2].tolist() == [0, 1] and sorted_loop.match_row[:2].tolist() == [1, -1]
    assert not np.array_equal(sorted_loop.match_row, got.match_row)


def test_5000_titles_on_one_row():
    got = check(ac.hot_row(), "hot row")
    assert (got.first_row == 0).all() and (got.match_row == 0).sum() == 1 and got.counts[1] == 65


def test_random_ties_under_both_options_at_their_extremes(random_ties, option):
    case, want = random_ties
    first = check(case, "defaults", expected=want)
    assert first.counts[2] > 1000 and first.counts[5] >= 2
    for blocks, rounds in ((1, 8), (0, 1), (1, 1), (3, 1024)):
        option("max_blocks", blocks)
        option("rounds_per_sync", rounds)
        got = check(case, (blocks, rounds), expected=want)
        assert all(np.array_equal(a, b) for a, b in zip(got[:3], first[:3]))
        assert np.array_equal(got.counts[:4], first.counts[:4])


def test_the_same_edges_in_one_chunk_and_in_several(random_ties):
    case, want = random_ties
    count = case.row.shape[0]
    whole = check(case, "one chunk", expected=want)
    for at in ((7,), (4096,), (count - 1,), (7, 4096, count - 1)):
        got = check(case, at, at=at, expected=want)
        assert all(np.array_equal(a, b) for a, b in zip(got[:3], whole[:3]))
        assert np.array_equal(got.counts[:4], whole.counts[:4])


@pytest.mark.parametrize("name", ["n_truth_1", "n_1", "one_title", "odd_count"])
def test_sizes_at_the_edges(name):
    got = check(ac.ALL[name](), name)
    if name == "n_truth_1":
        assert (got.match_row >= 0).sum() == 1


def test_no_title_launches_nothing_and_leaves_zero_counts():
    case = ac.small(0, 3, 10)
    keys, rows, got = run(case)
    assert got.counts.tolist() == [0] * 6 and got.match_row.shape == (0,)
    from doppel_speller_amd import _lib
    # nothing was written: not the keys, not the state
    key, state = _lib.DeviceArray.from_host(np.full((1, 3), 7, np.uint64)), _lib.DeviceArray.from_host(np.full(10, 7, np.uint64))
    some = [_lib.DeviceArray.from_host(np.full(1, 7, np.int32)) for _ in range(5)]
    counts = _lib.DeviceArray.from_host(np.full(6, -1, np.int64))
    assert _lib.lib().ds_assign_solve_device(some[0].ptr, key.ptr, 0, 3, 10, state.ptr, *(a.ptr for a in some[1:]),
                                             counts.ptr, ctypes.c_void_p(0)) == 0
    assert (state.to_host() == 7).all() and all((a.to_host() == 7).all() for a in some) and not counts.to_host().any()


def test_no_truth_row():
    """n_truth = 0: no slot can be an edge, every title comes back empty."""
    case = ac.small(100, 2, 5)._replace(n_truth=0)
    got = check(case, "n_truth = 0")
    assert (got.match_row == -1).all() and (got.first_row == -1).all() and got.counts.tolist() == [0, 0, 0, 0, 0, 1]


def test_keys_with_rows_outside_the_truth_set_are_no_edges_for_the_solver():
    """The solver takes keys from any caller: a non-zero key on a row outside [0, n_truth) must index nothing."""
    from doppel_speller_amd import _lib
    case = ac.small(500, 3, 50)
    keys = ac.keys_of(case)
    rows = case.row.copy()
    rows[::7, 1], rows[3::11, 0] = 50, -1                                   # the keys stay
    want = ac.deferred_acceptance(rows, keys, 50)
    d_rows, d_keys = _lib.DeviceArray.from_host(rows), _lib.DeviceArray.from_host(keys)
    held = _lib.DeviceArray((50,), np.uint64)
    outputs = [_lib.DeviceArray((500,), np.int32) for _ in range(4)]
    counts = _lib.DeviceArray((6,), np.int64)
    _lib.check(_lib.lib().ds_assign_solve_device(d_rows.ptr, d_keys.ptr, 500, 3, 50, held.ptr, *(a.ptr for a in outputs),
                                                 counts.ptr, ctypes.c_void_p(0)), "ds_assign_solve_device")
    for mine, theirs in zip(outputs[1:], want[:3]):
        assert np.array_equal(mine.to_host(), theirs)
    assert counts.to_host()[:4].tolist() == want.counts.tolist()


def test_bad_arguments_launch_nothing():
    from doppel_speller_amd import _lib
    lib = _lib.lib()
    case = ac.small(64, 4, 30)
    device = [_lib.DeviceArray.from_host(a) for a in case[:4]]
    keys = _lib.DeviceArray.from_host(np.full((64, 4), 7, dtype=np.uint64))
    rows = _lib.DeviceArray.from_host(np.full((64, 4), 7, dtype=np.int32))
    stream = ctypes.c_void_p(0)
    good = [a.ptr for a in device] + [0, 64, 64, 4, 30, 0.9, keys.ptr, rows.ptr, stream]
    for position, value in ((0, None), (1, None), (2, None), (3, None), (10, None), (11, None), (4, -1), (5, -1), (6, -1),
                            (5, 65), (4, 1), (6, 63), (6, 1 << 31), (7, 0), (7, -1), (8, -1), (8, 1 << 31),
                            (9, float("nan")), (9, float("inf")), (9, float("-inf"))):
        bad = list(good)
        bad[position] = ctypes.c_void_p(0) if value is None else value
        assert lib.ds_assign_edges_device(*bad) == -1, (position, value)
    _lib.check(lib.ds_stream_sync(None, 0), "sync")
    assert (keys.to_host() == 7).all() and (rows.to_host() == 7).all()

    held = _lib.DeviceArray.from_host(np.full(30, 7, dtype=np.uint64))
    outputs = [_lib.DeviceArray.from_host(np.full(64, 7, dtype=np.int32)) for _ in range(4)]
    counts = _lib.DeviceArray.from_host(np.full(6, 7, dtype=np.int64))
    good = [rows.ptr, keys.ptr, 64, 4, 30, held.ptr] + [a.ptr for a in outputs] + [counts.ptr, stream]
    for position, value in ((0, None), (1, None), (5, None), (6, None), (7, None), (8, None), (9, None), (10, None),
                            (2, -1), (2, 1 << 31), (3, 0), (3, -1), (4, -1), (4, 1 << 31)):
        bad = list(good)
        bad[position] = ctypes.c_void_p(0) if value is None else value
        assert lib.ds_assign_solve_device(*bad) == -1, (position, value)
    _lib.check(lib.ds_stream_sync(None, 0), "sync")
    assert (held.to_host() == 7).all() and (counts.to_host() == 7).all() and all((a.to_host() == 7).all() for a in outputs)
    for name, value in ((b"max_blocks", -1), (b"max_blocks", (1 << 20) + 1), (b"rounds_per_sync", 0),
                        (b"rounds_per_sync", 1025), (b"nothing", 1)):
        assert lib.ds_assign_option(name, value) == -1
