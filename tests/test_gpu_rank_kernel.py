"""ds_rank_matches_device through the C ABI against the NumPy restatement of the ranking rule (tests/ranked_cases.py),
bit for bit: both kernels (keys in LDS / selection from HBM), every situation of the rule, the launch limits, the
argument errors."""
import numpy as np
import pytest

import ranked_cases as rc
from doppel_speller_amd import _lib

pytestmark = pytest.mark.gpu

LDS_KEYS = 512                 # the most candidates ds_rank_lds_kernel holds (kRankLdsKeys)
QUERIES_PER_BLOCK = 4          # one wave per query, 256 threads (kRankWaves)
MAX_BLOCKS = 4096              # the grid is capped there and strides (kRankMaxBlocks)


@pytest.fixture
def lds_keys():
    """Sets the "lds_keys" limit for a test and puts the default back."""
    def choose(value):
        _lib.check(_lib.lib().ds_rank_option(b"lds_keys", value), "ds_rank_option")
    yield choose
    choose(LDS_KEYS)


def _rank(rows, probabilities, ratios, exact, best, n, n_truth):
    n_queries, k = rows.shape
    device = [_lib.DeviceArray.from_host(a) if a is not None and a.size else None
              for a in (rows, probabilities, ratios, exact, best)]
    if n_queries == 0:                  # nothing is read or written: any non-null address will do
        device[:3] = [_lib.DeviceArray((1,), np.int32)] * 3
    outputs = [_lib.DeviceArray((max(1, n_queries * n),), dtype) for dtype in (np.int32, np.float32, np.uint8, np.int8)]
    for out in outputs:                 # a slot the kernel leaves out shows as 0x55 bytes
        _lib.check(_lib.lib().ds_memset(out.ptr, 0x55, out.nbytes, 0), "ds_memset")
    _lib.check(_lib.lib().ds_rank_matches_device(*(_lib.pointer(a) for a in device), n_queries, k, n, n_truth,
                                                 *(a.ptr for a in outputs), _lib.pointer(None)),
               "ds_rank_matches_device")
    _lib.check(_lib.lib().ds_stream_sync(_lib.pointer(None), 0), "sync")
    return tuple(a.to_host(n_queries * n).reshape(n_queries, n) for a in outputs)


def _check(groups, n, n_truth, what):
    got = _rank(*groups, n, n_truth)
    assert rc.same_ranking(got, rc.rank_matches(*groups, n, n_truth)), what
    return got


@pytest.mark.parametrize("k", [1, 5, 10, 17, 64, 100, 128, 1000])
def test_every_k_on_both_paths(k, lds_keys):
    """k = 1000 does not fit the LDS kernel and takes the selection kernel on its own; every other k runs on both, the
    selection kernel forced with lds_keys = 0, and the two answers are the same bits."""
    n_truth = 2 * k + 2
    for ties in ("none", "some", "all", "k"):
        groups = rc.make_groups(203, k, n_truth, seed=k, ties=ties)
        for n in sorted({1, min(3, k), k}):
            lds_keys(LDS_KEYS)
            first = _check(groups, n, n_truth, (k, ties, n, "default"))
            lds_keys(0)
            assert rc.same_ranking(first, _check(groups, n, n_truth, (k, ties, n, "select"))), (k, ties, n)


def test_the_limit_between_the_paths(lds_keys):
    for k in (LDS_KEYS, LDS_KEYS + 1):
        n_truth = 2 * k + 2
        groups = rc.make_groups(19, k, n_truth, seed=k)
        for n in (1, 3, k):
            _check(groups, n, n_truth, (k, n))
    groups = rc.make_groups(19, 100, 202, seed=5)
    for limit in (99, 100):             # the selection kernel, then the LDS kernel, at a limit of the caller's
        lds_keys(limit)
        _check(groups, 7, 202, limit)


def test_null_exact_and_null_best(lds_keys):
    rows, probabilities, ratios, exact, best = rc.make_groups(64, 17, 40, seed=3)
    for limit in (LDS_KEYS, 0):
        lds_keys(limit)
        for exact_, best_ in ((None, best), (exact, None), (None, None)):
            _check((rows, probabilities, ratios, exact_, best_), 5, 40, (limit, exact_ is None, best_ is None))


@pytest.mark.parametrize("n_queries", [0, 1, QUERIES_PER_BLOCK * MAX_BLOCKS + 5, QUERIES_PER_BLOCK * 65535 + 6])
def test_query_counts_past_the_grid(n_queries, lds_keys):
    """One wave per query, four per workgroup, at most 4096 workgroups that stride over the rest: a count past the cap,
    and one past 65,535 workgroups' worth, on both kernels."""
    groups = rc.make_groups(n_queries, 5, 12, seed=n_queries % 1000, ties="some")
    expected = rc.rank_matches(*groups, 3, 12)
    for limit in (LDS_KEYS, 0):
        lds_keys(limit)
        got = _rank(*groups, 3, 12)
        assert got[0].shape == (n_queries, 3) and rc.same_ranking(got, expected), limit


def test_argument_errors(lds_keys):
    rows, probabilities, ratios, exact, best = rc.make_groups(8, 5, 12, seed=1)
    device = [_lib.DeviceArray.from_host(a) for a in (rows, probabilities, ratios, exact, best)]
    outputs = [_lib.DeviceArray((8 * 5,), dtype) for dtype in (np.int32, np.float32, np.uint8, np.int8)]
    pointers = [a.ptr for a in device] + [8, 5, 3, 12] + [a.ptr for a in outputs] + [_lib.pointer(None)]
    call = _lib.lib().ds_rank_matches_device
    assert call(*pointers) == 0
    for position in (0, 1, 2, 9, 10, 11, 12):                          # every pointer but exact, best and the stream
        bad = list(pointers)
        bad[position] = _lib.pointer(None)
        assert call(*bad) == -1, position
        assert b"null" in _lib.lib().ds_last_error()
    for position, value in ((6, 0), (6, -1), (7, 0), (7, 6), (7, -2), (5, -1), (8, -1)):   # k, n, the two counts
        bad = list(pointers)
        bad[position] = value
        assert call(*bad) == -1, (position, value)
    empty = list(pointers)
    empty[5] = 0
    assert call(*empty) == 0
    option = _lib.lib().ds_rank_option
    assert option(b"lds_keys", LDS_KEYS + 1) == -1 and option(b"lds_keys", -1) == -1
    assert option(b"no_such_option", 1) == -1 and option(None, 1) == -1
    _lib.check(_lib.lib().ds_stream_sync(_lib.pointer(None), 0), "sync")
