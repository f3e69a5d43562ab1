"""ds_close_parts_device and ds_threshold_sweep_device through the C ABI against the restatement of tests/sweep_cases.py,
bit for bit: the three parts of the close ratio on hostile titles (tests/title_cases.py) read at every threshold of their
range, the sweep's counters on synthetic queries at every size where the kernel takes another path, the accumulation over
calls, the argument errors."""
import ctypes

import numpy as np
import pytest

import sweep_cases as sc
import title_cases as tc

pytestmark = pytest.mark.gpu

SENTINEL = 0xee                # 238: no part (0..100)
WAVES = 4                      # queries per workgroup and pass (kSweepWaves)
MAX_GROUPS = 256               # workgroups along the queries at most (kSweepMaxBlocks)
N_TRUTH = 1000


# ---- the close ratio taken apart ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tables():
    from doppel_speller_amd import _lib
    from doppel_speller_amd.feature_engineering import SORT_KEY, TitleTable
    case = tc.close_case()
    return case, TitleTable(case.q_enc, case.q_len), TitleTable(case.t_enc, case.t_len, case.t_counts), \
        _lib.DeviceArray.from_host(SORT_KEY), SORT_KEY


def close_parts(queries, truth, d_sort_key, rows, q_first, t_min, t_max):
    from doppel_speller_amd import _lib
    lib = _lib.lib()
    n_queries, k = rows.shape
    d_rows = _lib.DeviceArray.from_host(np.ascontiguousarray(rows, dtype=np.int32))
    outputs = [_lib.DeviceArray((n_queries, k), np.uint8) for _ in range(3)]
    for out in outputs:
        _lib.check(lib.ds_memset(out.ptr, SENTINEL, out.nbytes, 0), "ds_memset")
    _lib.check(lib.ds_close_parts_device(queries.handle, truth.handle, d_rows.ptr, q_first, k, n_queries, tc.SPACE,
                                         d_sort_key.ptr, t_min, t_max, *(out.ptr for out in outputs), ctypes.c_void_p(0)),
               "ds_close_parts_device")
    _lib.check(lib.ds_stream_sync(None, 0), "sync")
    return tuple(out.to_host() for out in outputs)


@pytest.fixture(scope="module")
def expected_parts(oracle, tables):
    """(rows of the two launches, their pairs, the restated parts of all pairs), shared by the ranges."""
    from doppel_speller_amd.feature_engineering import TitleTable
    case, _, _, _, sort_key = tables
    pair_q, pair_t = sc.close_pairs(case)
    hostile = pair_t[:3000].reshape(300, 10).astype(np.int32)          # queries 0..299 of the table
    q_special = tc.special_rows(case.q_enc, case.q_len, case.q_large)
    special = pair_t[3000:].reshape(q_special.shape[0], -1).astype(np.int32)
    special_queries = TitleTable(case.q_enc[q_special], case.q_len[q_special])   # the rows form reads consecutive rows
    return hostile, special, special_queries, pair_q, pair_t, sc.case_parts(oracle, case, pair_q, pair_t, sort_key)


@pytest.mark.parametrize("t_min, t_max", [(0, 100), (94, 94)])
def test_close_parts(oracle, tables, expected_parts, t_min, t_max):
    case, queries, truth, d_sort_key, sort_key = tables
    hostile, special, special_queries, pair_q, pair_t, full = expected_parts
    got = [np.concatenate((a.reshape(-1), b.reshape(-1))) for a, b in zip(
        close_parts(queries, truth, d_sort_key, hostile, 0, t_min, t_max),
        close_parts(special_queries, truth, d_sort_key, special, 0, t_min, t_max))]
    for name, mine, theirs in zip("drs", got, sc.skipped_parts(*full, t_min, t_max)):
        wrong = np.nonzero(mine != theirs)[0]
        assert wrong.shape[0] == 0, (name, wrong.shape[0], wrong[:5], mine[wrong][:5], theirs[wrong][:5],
                                     pair_q[wrong][:5], pair_t[wrong][:5])
    for t in range(t_min, t_max + 1):          # the parent's own ratio at every threshold of the range
        assert np.array_equal(sc.value_at(*got, t), tc.expected_ratios(oracle, case, pair_q, pair_t, t, sort_key)), t
    d, r, s = full
    skipped = d < t_min
    assert skipped.any() == (t_min > 0) and not got[1][skipped].any() and not got[2][skipped].any()
    assert ((r > t_max) & ~skipped).any() == (t_max < 100) and not got[2][(r > t_max) & ~skipped].any()


def test_close_parts_argument_errors(tables):
    from doppel_speller_amd import _lib
    _, queries, truth, d_sort_key, _ = tables
    rows = _lib.DeviceArray.from_host(np.zeros((4, 3), dtype=np.int32))
    outputs = [_lib.DeviceArray((4, 3), np.uint8) for _ in range(3)]
    arguments = [queries.handle, truth.handle, rows.ptr, 0, 3, 4, tc.SPACE, d_sort_key.ptr, 0, 100] + \
        [out.ptr for out in outputs] + [ctypes.c_void_p(0)]
    call = _lib.lib().ds_close_parts_device
    assert call(*arguments) == 0
    for position in (0, 1, 2, 7, 10, 11, 12):
        bad = list(arguments)
        bad[position] = ctypes.c_void_p(0)
        assert call(*bad) == -1, position
        assert b"null" in _lib.lib().ds_last_error()
    for position, value in ((4, 0), (5, -1), (8, -1), (9, 101), (8, 95)):      # k, the count, the range (95 > t_max = 94)
        bad = list(arguments)
        bad[9] = 94 if position == 8 and value == 95 else bad[9]
        bad[position] = value
        assert call(*bad) == -1, (position, value)
    empty = list(arguments)
    empty[5] = 0
    assert call(*empty) == 0
    _lib.check(_lib.lib().ds_stream_sync(None, 0), "sync")


# ---- the sweep ------------------------------------------------------------------------------------------------------

@pytest.fixture
def queries_per_group():
    """Sets the "queries_per_group" option for a test and puts the default back."""
    from doppel_speller_amd import _lib

    def choose(value):
        _lib.check(_lib.lib().ds_sweep_option(b"queries_per_group", value), "ds_sweep_option")
    yield choose
    choose(0)


def sweep(queries, lev, prob, counts=None):
    """One ds_threshold_sweep_device call on host arrays -> int64[T, U, 4], added to `counts` when given."""
    from doppel_speller_amd import _lib
    lib = _lib.lib()
    n_queries, k = queries[0].shape
    device = [_lib.DeviceArray.from_host(a) if a.size else _lib.DeviceArray((1,), a.dtype) for a in queries]
    d_lev, d_prob = _lib.DeviceArray.from_host(lev), _lib.DeviceArray.from_host(prob)
    start = np.zeros((lev.shape[0], prob.shape[0], 4), dtype=np.int64) if counts is None else counts
    d_counts = _lib.DeviceArray.from_host(start)
    _lib.check(lib.ds_threshold_sweep_device(*(a.ptr for a in device), n_queries, k, d_lev.ptr, lev.shape[0], d_prob.ptr,
                                             prob.shape[0], d_counts.ptr, ctypes.c_void_p(0)), "ds_threshold_sweep_device")
    _lib.check(lib.ds_stream_sync(None, 0), "sync")
    return d_counts.to_host()


def check(oracle, queries, lev, prob, what):
    expected = sc.sweep_counts(oracle, queries, lev, prob)
    got = sweep(queries, lev, prob)
    wrong = np.argwhere(got != expected)
    assert wrong.shape[0] == 0, (what, wrong.shape[0], wrong[:5], got[tuple(wrong[:5].T)], expected[tuple(wrong[:5].T)])
    assert (got.sum(axis=-1) == queries[0].shape[0]).all()
    return got


@pytest.mark.parametrize("shape", [(1, 1), (3, 7), (101, 256)])
@pytest.mark.parametrize("k", [1, 5, 100])
def test_every_size_and_grid(oracle, k, shape):
    """n_queries 1, 257 (five workgroups, thirteen passes each) and 16,389 (past 256 workgroups x 64 queries: the cap, and
    every workgroup strides); T x U from one cell to the largest grid, which takes seven tiles of thresholds."""
    lev, prob = sc.GRID_3X7 if shape == (3, 7) else sc.grid(*shape)
    sizes = (1, 257, MAX_GROUPS * 64 + 5) if shape == (3, 7) else (1, 257)
    for n_queries in sizes:
        queries = sc.make_queries(n_queries, k, N_TRUTH, seed=100 * k + shape[0])
        got = check(oracle, queries, lev, prob, (k, shape, n_queries))
        if n_queries >= 257:
            assert (got.reshape(-1, 4).max(axis=0) > 0).all()            # every outcome occurs


def test_crafted_queries_alone(oracle):
    lev, prob = sc.GRID_3X7
    for k in (5, 100):
        queries = sc.crafted_queries(k)
        got = check(oracle, queries, lev, prob, k)
        assert got[0, 0].tolist() == [3, 3, 1, 0] and got[2, 6].tolist() == [2, 1, 1, 3]


def test_the_cap_of_the_grid_at_a_small_size(oracle, queries_per_group):
    """Four queries per workgroup: 1,029 queries reach the cap of 256 workgroups, and the first of them strides."""
    lev, prob = sc.grid(20, 50)
    queries = sc.make_queries(MAX_GROUPS * WAVES + 5, 5, N_TRUTH, seed=9)
    first = check(oracle, queries, lev, prob, "default")
    for per_group in (4, 1, 1 << 30):
        queries_per_group(per_group)
        assert np.array_equal(first, check(oracle, queries, lev, prob, per_group))


def test_two_calls_on_two_halves_add_up(oracle):
    lev, prob = sc.grid(20, 50)
    queries = sc.make_queries(600, 5, N_TRUTH, seed=4)
    whole = check(oracle, queries, lev, prob, "whole")
    counts = sweep(tuple(a[:257] for a in queries), lev, prob)
    counts = sweep(tuple(a[257:] for a in queries), lev, prob, counts)
    assert np.array_equal(counts, whole)
    assert np.array_equal(sweep(tuple(a[:0] for a in queries), lev, prob, counts), whole)     # no queries: nothing added


def test_nan_probabilities_follow_the_sequential_scan(oracle):
    """ds_select_matches_kernel starts from the first candidate and compares: a NaN in front stays (no match), a NaN behind
    it never wins.  oracle.select_matches (np.max) agrees only on the first, so the second is stated here."""
    rows = np.array([[3, 4, 5], [6, 7, 8]], dtype=np.int32)
    zero = np.zeros((2, 3), dtype=np.uint8)
    p = np.array([[np.nan, 0.99, 0.5], [0.5, np.nan, 0.99]], dtype=np.float32)
    none = np.full(2, -1, dtype=np.int32)
    lev, prob = sc.grid(1, 1)
    got = sweep((rows, zero, zero, zero, p, none, np.array([4, 8], dtype=np.int32)), lev, prob)
    assert got[0, 0].tolist() == [1, 0, 0, 1]


def test_argument_errors():
    from doppel_speller_amd import _lib
    queries = sc.make_queries(8, 5, N_TRUTH, seed=1)
    device = [_lib.DeviceArray.from_host(a) for a in queries]
    lev, prob = sc.GRID_3X7
    d_lev, d_prob = _lib.DeviceArray.from_host(lev), _lib.DeviceArray.from_host(prob)
    d_counts = _lib.DeviceArray.from_host(np.zeros(3 * 7 * 4, dtype=np.int64))
    arguments = [a.ptr for a in device] + [8, 5, d_lev.ptr, 3, d_prob.ptr, 7, d_counts.ptr, ctypes.c_void_p(0)]
    call = _lib.lib().ds_threshold_sweep_device
    assert call(*arguments) == 0
    for position in (0, 1, 2, 3, 4, 5, 6, 9, 11, 13):                  # every pointer but the stream
        bad = list(arguments)
        bad[position] = ctypes.c_void_p(0)
        assert call(*bad) == -1, position
        assert b"null" in _lib.lib().ds_last_error()
    for position, value in ((7, -1), (8, 0), (8, -3), (10, 0), (10, 102), (12, 0), (12, 257)):   # the count, k, T, U
        bad = list(arguments)
        bad[position] = value
        assert call(*bad) == -1, (position, value)
    for bad_lev in ([50, 50, 94], [90, 50, 94], [-1, 50, 94], [50, 94, 101]):
        bad = list(arguments)
        held = _lib.DeviceArray.from_host(np.array(bad_lev, dtype=np.int32))
        bad[9] = held.ptr
        assert call(*bad) == -1 and b"Levenshtein" in _lib.lib().ds_last_error(), bad_lev
    for bad_prob in ([.1, .2, .3, .3, .5, .6, .7], [.1, .2, .3, .25, .5, .6, .7], [.1, .2, .3, .4, .5, .6, np.inf],
                     [np.nan, .2, .3, .4, .5, .6, .7], [-np.inf, .2, .3, .4, .5, .6, .7]):
        bad = list(arguments)
        held = _lib.DeviceArray.from_host(np.array(bad_prob, dtype=np.float32))
        bad[11] = held.ptr
        assert call(*bad) == -1 and b"probability" in _lib.lib().ds_last_error(), bad_prob
    _lib.check(_lib.lib().ds_stream_sync(None, 0), "sync")
    assert np.array_equal(d_counts.to_host().reshape(3, 7, 4).sum(axis=-1), np.full((3, 7), 8))    # the one good call only
    empty = list(arguments)
    empty[7] = 0
    assert call(*empty) == 0
    option = _lib.lib().ds_sweep_option
    assert option(b"queries_per_group", -1) == -1 and option(b"queries_per_group", (1 << 30) + 1) == -1
    assert option(b"no_such_option", 1) == -1 and option(None, 1) == -1
