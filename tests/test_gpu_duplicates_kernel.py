"""ds_duplicate_begin_device, ds_duplicate_links_device and ds_duplicate_finish_device through the C ABI on the link sets
of tests/duplicates_cases.py -- the shapes where a concurrent union-find goes wrong -- against the restatement there, bit
for bit: labels, sizes, reasons and counters, and the invariant of the forest (parent[i] <= i, every entry at its root after
the finish)."""
import ctypes

import numpy as np
import pytest

import duplicates_cases as dc

pytestmark = pytest.mark.gpu

SENTINEL = 0xee                # no reason (0..3)


def run(calls, n_truth, t=dc.T, u=dc.U, reasons=True):
    """begin, one links call per entry of `calls`, finish -> (labels, sizes, [reasons per call], counts, parent)."""
    from doppel_speller_amd import _lib
    lib = _lib.lib()
    stream = ctypes.c_void_p(0)
    parent = _lib.DeviceArray((max(n_truth, 1),), np.int32)
    counts = _lib.DeviceArray.from_host(np.full(3, -77, dtype=np.int64))              # begin zeroes them
    _lib.check(lib.ds_memset(parent.ptr, SENTINEL, parent.nbytes, 0), "ds_memset")
    _lib.check(lib.ds_duplicate_begin_device(parent.ptr, n_truth, counts.ptr, stream), "ds_duplicate_begin_device")
    held = []
    for q_first, rows, ratios, probabilities, exact in calls:
        n_queries, k = rows.shape
        device = [None if a is None else (_lib.DeviceArray.from_host(a) if a.size else _lib.DeviceArray((1,), a.dtype))
                  for a in (rows, ratios, probabilities, exact)]
        d_reason = None
        if reasons:
            d_reason = _lib.DeviceArray((max(n_queries, 1), k), np.uint8)
            _lib.check(lib.ds_memset(d_reason.ptr, SENTINEL, d_reason.nbytes, 0), "ds_memset")
        _lib.check(lib.ds_duplicate_links_device(*(_lib.pointer(a) for a in device), q_first, n_queries, k, n_truth, int(t),
                                                 float(u), parent.ptr, _lib.pointer(d_reason), counts.ptr, stream),
                   "ds_duplicate_links_device")
        held.append((device, d_reason, n_queries))
    labels, sizes = (_lib.DeviceArray((max(n_truth, 1),), np.int32) for _ in range(2))
    for out in (labels, sizes):
        _lib.check(lib.ds_memset(out.ptr, SENTINEL, out.nbytes, 0), "ds_memset")
    _lib.check(lib.ds_duplicate_finish_device(parent.ptr, n_truth, labels.ptr, sizes.ptr, stream), "ds_duplicate_finish_device")
    _lib.check(lib.ds_stream_sync(None, 0), "sync")
    return (labels.to_host(n_truth), sizes.to_host(n_truth),
            [None if d_reason is None else d_reason.to_host(n_queries) for _, d_reason, n_queries in held],
            counts.to_host(), parent.to_host(n_truth))


def check(calls, n_truth, what, t=dc.T, u=dc.U, reasons=True):
    labels, sizes, call_reasons, counts = dc.expected(calls, n_truth, t, u)
    got = run(calls, n_truth, t, u, reasons)
    wrong = np.nonzero(got[0] != labels)[0]
    assert wrong.shape[0] == 0, (what, "labels", wrong.shape[0], wrong[:5], got[0][wrong][:5], labels[wrong][:5])
    wrong = np.nonzero(got[1] != sizes)[0]
    assert wrong.shape[0] == 0, (what, "sizes", wrong.shape[0], wrong[:5], got[1][wrong][:5], sizes[wrong][:5])
    assert got[3].tolist() == counts.tolist(), (what, "counts")
    for mine, theirs in zip(got[2], call_reasons):
        assert (mine is None) == (not reasons)
        if reasons:
            assert mine.dtype == np.uint8 and np.array_equal(mine, theirs), (what, "reasons", np.argwhere(mine != theirs)[:5])
    assert np.array_equal(got[4], labels), (what, "the forest is not compressed to its roots")
    return got


@pytest.fixture
def max_blocks():
    """Sets the "max_blocks" option for a test and puts the default back."""
    from doppel_speller_amd import _lib

    def choose(value):
        _lib.check(_lib.lib().ds_duplicates_option(b"max_blocks", value), "ds_duplicates_option")
    yield choose
    choose(0)


@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_a_chain_of_100000_rows(order):
    """Deep trees, and hooks racing along one path: 391 workgroups at work on one component."""
    labels, sizes, _, counts, _ = check(dc.chain(100_000, order), 100_000, order)
    assert not labels.any() and (sizes == 100_000).all() and counts.tolist() == [0, 99_999, 0]


@pytest.mark.parametrize("centre", [0, 19_999])
def test_a_star_of_20000_rows(centre):
    """Every compare-and-swap contends on one root; with the centre in the LAST row the root must still end at row 0."""
    labels, sizes, _, _, _ = check(dc.star(20_000, centre), 20_000, centre)
    assert not labels.any() and (sizes == 20_000).all()


def test_two_components_joined_by_a_link_of_a_later_call():
    calls = dc.two_halves_joined_later(30_000)
    labels, sizes, _, _, _ = check(calls[:1], 60_000, "the halves")
    assert sorted(set(labels.tolist())) == [0, 30_000] and (sizes == 30_000).all()
    labels, sizes, _, _, _ = check(calls, 60_000, "joined")
    assert not labels.any() and (sizes == 60_000).all()


def test_the_same_links_in_one_three_and_seven_calls():
    n, k = 20_000, 5
    whole = dc.random_links(n, k, seed=21)
    first = check(whole, n, "whole")
    assert (first[3] > 0).all() and 1 in first[1] and first[1].max() > 100
    for pieces in (3, 7):
        parts = dc.cut(whole[0], pieces)
        got = check(parts, n, pieces)
        assert np.array_equal(got[0], first[0]) and np.array_equal(got[1], first[1]) and np.array_equal(got[3], first[3])
        assert np.array_equal(np.concatenate(got[2]), first[2][0])
    # the pieces in another order, and one of them twice: the components and the reasons stay, the counters add up
    parts = dc.cut(whole[0], 7)
    again = run(parts[::-1] + parts[2:3], n)
    assert np.array_equal(again[0], first[0]) and np.array_equal(again[1], first[1])
    assert (again[3] > first[3]).all()


def test_many_small_components():
    n = 30_000
    check(dc.random_links(n, 3, seed=8, block=7, share=0.3), n, "blocks of seven")


def test_every_row_linked_to_every_candidate_at_k_64():
    n = 5_000
    labels, sizes, _, counts, _ = check(dc.dense(n), n, "dense")
    assert sorted(set(labels.tolist())) == list(range(0, n, 500)) and (sizes == 500).all()
    assert counts[1] >= n * 64 - n * 64 // 400                     # all but the slots that drew the own row


def test_identical_titles_through_the_exact_rows_alone():
    labels, sizes, (reasons,), counts, _ = check(dc.twins(20_000), 20_000, "twins")
    assert not labels.any() and (sizes == 20_000).all() and counts.tolist() == [19_999, 0, 0] and not reasons.any()


def test_no_link_at_all():
    labels, sizes, (reasons,), counts, _ = check(dc.nothing(5_000), 5_000, "nothing")
    assert labels.tolist() == list(range(5_000)) and (sizes == 1).all() and not counts.any() and not reasons.any()


def test_skipped_slots_and_values_at_the_thresholds():
    labels, sizes, (reasons,), counts, _ = check(dc.edge_slots(), 300, "edges")
    assert reasons[2].tolist() == [0, 1, 0, 0, 1, 0, 1, 0] and reasons[3].tolist() == [0, 2, 0, 0, 2, 0, 0, 2]
    assert counts.tolist() == [2, 5, 5] and (sizes > 1).sum() == 15
    # other thresholds on the same slots: 0 and 100, and a probability threshold below every probability
    for t, u in ((0, 0.0), (100, -1.0), (93, float(np.nextafter(dc.U, np.float32(0))))):
        check(dc.edge_slots(), 300, (t, u), t=t, u=u)


def test_one_truth_row_no_queries_and_no_reason_buffer():
    one = [(0, np.zeros((1, 3), np.int32), np.full((1, 3), 100, np.uint8), np.ones((1, 3), np.float32), np.zeros(1, np.int32))]
    labels, sizes, (reasons,), counts, _ = check(one, 1, "n_truth = 1")
    assert labels.tolist() == [0] and sizes.tolist() == [1] and not reasons.any() and not counts.any()
    none = [(7, np.zeros((0, 4), np.int32), np.zeros((0, 4), np.uint8), None, None)]
    labels, sizes, _, counts, _ = check(none, 50, "n_queries = 0")
    assert labels.tolist() == list(range(50)) and (sizes == 1).all() and not counts.any()
    for calls, n in ((dc.random_links(3_000, 4, seed=2), 3_000), (dc.edge_slots(), 300), (dc.twins(500), 500)):
        check(calls, n, "d_reason NULL", reasons=False)


def test_the_cap_of_the_grids_at_its_extremes(max_blocks):
    """One workgroup strides over everything; 2^20 leaves every grid as large as its input asks."""
    n = 20_000
    whole = dc.random_links(n, 5, seed=21)
    first = check(whole, n, "default")
    chain = check(dc.chain(30_000, "shuffled"), 30_000, "default")
    for cap in (1, 3, 1 << 20):
        max_blocks(cap)
        got = check(whole, n, cap)
        assert all(np.array_equal(a, b) for a, b in zip(got[:2] + got[3:], first[:2] + first[3:]))
        assert np.array_equal(check(dc.chain(30_000, "shuffled"), 30_000, cap)[0], chain[0])
        check(dc.cut(whole[0], 3), n, (cap, 3))


def test_bad_arguments_launch_nothing():
    from doppel_speller_amd import _lib
    lib = _lib.lib()
    (q_first, rows, ratios, probabilities, exact), = dc.random_links(64, 4, seed=1)
    device = [_lib.DeviceArray.from_host(a) for a in (rows, ratios, probabilities, exact)]
    parent, counts = _lib.DeviceArray((64,), np.int32), _lib.DeviceArray((3,), np.int64)
    reason = _lib.DeviceArray.from_host(np.full((64, 4), SENTINEL, dtype=np.uint8))
    stream = ctypes.c_void_p(0)
    assert lib.ds_duplicate_begin_device(parent.ptr, 64, counts.ptr, stream) == 0
    good = [a.ptr for a in device] + [0, 64, 4, 64, 94, 0.9, parent.ptr, reason.ptr, counts.ptr, stream]
    for position, value in ((0, None), (1, None), (10, None), (12, None), (4, -1), (5, -1), (5, 65), (4, 1), (6, 0),
                            (7, -1), (8, 101), (8, -1), (9, float("nan")), (9, float("inf"))):
        bad = list(good)
        bad[position] = ctypes.c_void_p(0) if value is None else value
        assert lib.ds_duplicate_links_device(*bad) == -1, (position, value)
    _lib.check(lib.ds_stream_sync(None, 0), "sync")
    assert parent.to_host().tolist() == list(range(64)) and not counts.to_host().any()
    assert (reason.to_host() == SENTINEL).all()
    # the pointers that may be NULL
    for position in (2, 3, 11):
        fine = list(good)
        fine[position] = ctypes.c_void_p(0)
        assert lib.ds_duplicate_links_device(*fine) == 0, position
    _lib.check(lib.ds_stream_sync(None, 0), "sync")
    assert (parent.to_host() <= np.arange(64)).all()
