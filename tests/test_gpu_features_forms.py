"""ds_construct_features_kernel in every launch form on hostile titles (tests/title_cases.py), all 66 values of every pair
against oracle.construct_features bit for bit; a pair outside the tables is 66 x 0x7fc00000.  Every output buffer is
filled with a finite sentinel in front of the launch: a row the kernel skipped is a failure, not a lucky NaN.
tests/test_title_cases_cpu.py pins, from the inputs alone, that these cases reach the paths the tests are named for:
a literal pair next to a bit-parallel one inside one staged query's run, units that cover two queries (k = 17, 23, 127),
rows outside the tables."""
import ctypes

import numpy as np
import pytest

import title_cases as tc

pytestmark = pytest.mark.gpu

SENTINEL_BYTE = 0x3b                     # float32 0x3b3b3b3b = 0.00286: finite, and no value construct_features produces
SENTINEL = 0x3b3b3b3b


class Tables:
    def __init__(self, case):
        from doppel_speller_amd.feature_engineering import TitleTable
        self.case = case
        self.queries = TitleTable(case.q_enc, case.q_len)
        self.truth = TitleTable(case.t_enc, case.t_len, case.t_counts)


@pytest.fixture(scope="module")
def tables():
    return Tables(tc.forms_case())


def filled_output(rows):
    """float32[rows, 66] in HBM, every byte the sentinel, the fill complete on return."""
    from doppel_speller_amd import _lib
    out = _lib.DeviceArray((rows, tc.FEATURES), np.float32)
    _lib.check(_lib.lib().ds_memset(out.ptr, SENTINEL_BYTE, out.nbytes, 0), "ds_memset")
    _lib.check(_lib.lib().ds_stream_sync(None, 0), "sync")
    return out


def enqueue(tables, d_q, d_t, q_first, k, n, n_truth, space, out, stream):
    """ds_construct_features_indexed_device and nothing else: no allocation, no fill, no synchronisation."""
    from doppel_speller_amd import _lib
    _lib.check(_lib.lib().ds_construct_features_indexed_device(
        tables.queries.handle, tables.truth.handle, _lib.pointer(d_q), d_t.ptr, q_first, k, space, n_truth, n, out.ptr,
        _lib.pointer(stream)), "ds_construct_features_indexed_device")


def launch(tables, pair_q, pair_t, q_first, k, n, n_truth=tc.N_TRUTH, space=tc.SPACE, room=None, stream=None):
    """One ds_construct_features_indexed_device launch -> uint32[room, 66] (room >= n rows, sentinel-filled in front).
    pair_q None: the rows form (d_pair_q = NULL, pair i belongs to query q_first + i / k)."""
    from doppel_speller_amd import _lib
    d_t = pair_t if isinstance(pair_t, _lib.DeviceArray) else _lib.DeviceArray.from_host(np.asarray(pair_t, dtype=np.int32))
    d_q = None
    if pair_q is not None:
        d_q = pair_q if isinstance(pair_q, _lib.DeviceArray) else _lib.DeviceArray.from_host(np.asarray(pair_q, dtype=np.int32))
    out = filled_output(room if room is not None else n)
    enqueue(tables, d_q, d_t, q_first, k, n, n_truth, space, out, stream)
    _lib.check(_lib.lib().ds_stream_sync(_lib.pointer(stream), 0), "sync")
    return out.to_host().view(np.uint32)


def assert_bits(got, expected, what):
    wrong = np.nonzero((got != expected).any(axis=1))[0]
    assert wrong.shape[0] == 0, (what, wrong.shape[0], wrong[:8].tolist(), got[wrong[0]].tolist(), expected[wrong[0]].tolist())


@pytest.mark.parametrize("k", tc.FEATURE_KS)
def test_rows_form(oracle, tables, k):
    """d_pair_q = NULL: q_first = 0 with every pair, then the LAST queries of the table with the launch cut inside the last
    query's run (the last unit is partial for every k > 1 -- a unit of one pair cannot be; the rows behind n keep the
    sentinel); with and without the truth records."""
    case = tables.case
    n_queries = tc.forms_queries(k)
    for q_first in (0, case.n_q - n_queries):
        rows = tc.forms_rows(case, k, q_first)
        pair_q, pair_t = tc.pairs_of_rows(rows, q_first)
        n = rows.size if q_first == 0 else rows.size - min(3, k - 1)
        expected = tc.expected_features(oracle, case, pair_q, pair_t)
        expected[n:] = SENTINEL
        for records in (1, 0, 1):
            tables.truth.option("truth_records", records)
            got = launch(tables, None, rows, q_first, k, n, room=rows.size)
            assert_bits(got, expected, (k, q_first, records))
    assert (expected[:n] == tc.NAN_BITS).all(axis=1).sum() >= n // 20      # rows outside the tables were among them


@pytest.mark.parametrize("k", [3, 10, 17])
def test_pair_list_of_the_remaining_queries(oracle, tables, k):
    """Explicit d_pair_q, as ds_remaining_pairs_device writes it from the same rows: runs of k per kept query, absolute
    query rows, units of 8 cutting through the runs; a best_row that drops a third of the queries."""
    from doppel_speller_amd import _lib
    lib = _lib.lib()
    case = tables.case
    n_queries = tc.forms_queries(k)
    q_first = case.n_q - n_queries
    rows = tc.forms_rows(case, k, q_first)
    best = np.where(np.arange(n_queries) % 3 == 1, 5, -1).astype(np.int32)
    d_best, d_rows = _lib.DeviceArray.from_host(best), _lib.DeviceArray.from_host(rows)
    d_q, d_t = _lib.DeviceArray((rows.size,), np.int32), _lib.DeviceArray((rows.size,), np.int32)
    counts = _lib.DeviceArray((int(lib.ds_remaining_pairs_counts_size(n_queries)),), np.int64)
    _lib.check(lib.ds_remaining_pairs_device(d_best.ptr, d_rows.ptr, n_queries, k, q_first, d_q.ptr, d_t.ptr, counts.ptr,
                                             ctypes.c_void_p(0)), "pairs")
    _lib.check(lib.ds_stream_sync(None, 0), "sync")
    n_remaining, n_pairs = (int(x) for x in counts.to_host()[:2])
    expected_q, expected_t = oracle.remaining_pairs(best, rows)
    assert n_remaining == int((best < 0).sum()) and n_pairs == n_remaining * k == expected_q.shape[0]
    assert np.array_equal(d_q.to_host()[:n_pairs], q_first + expected_q) and np.array_equal(d_t.to_host()[:n_pairs], expected_t)
    expected = tc.expected_features(oracle, case, q_first + expected_q.astype(np.int64), expected_t)
    for records in (1, 0, 1):
        tables.truth.option("truth_records", records)
        assert_bits(launch(tables, d_q, d_t, 0, 0, n_pairs), expected, (k, records))


def test_pair_list_shuffled_one_query_and_short(oracle, tables):
    """Explicit d_pair_q in no order at all (the staged query changes with every pair), with one query row throughout (it
    is staged once per unit), and n = 1, 7, 8, 9 and 8m + 1 pairs (units of 8)."""
    case = tables.case
    rows = tc.forms_rows(case, 7, 0)
    pair_q, pair_t = tc.pairs_of_rows(rows, 0)
    order = np.random.RandomState(4).permutation(pair_q.shape[0])
    pair_q, pair_t = pair_q[order], pair_t[order]
    pair_q[::29] = np.array([-1, case.n_q, tc.INT32_MAX])[np.arange(pair_q[::29].shape[0]) % 3]   # query rows outside, too
    expected = tc.expected_features(oracle, case, pair_q, pair_t)
    for records in (1, 0, 1):
        tables.truth.option("truth_records", records)
        for n in (1, 7, 8, 9, 8 * 50 + 1, pair_q.shape[0]):
            wanted = expected.copy()
            wanted[n:] = SENTINEL
            assert_bits(launch(tables, pair_q, pair_t, 0, 0, n, room=pair_q.shape[0]), wanted, (records, n))
    # one query row for every pair: a plain 129-character title with spaces, then an empty one
    plain = np.nonzero(~case.q_large & (case.q_len == 129))[0]
    for q in (int(plain[1]), int(np.nonzero(case.q_len == 0)[0][0])):
        same_q = np.full(pair_t.shape[0], q, dtype=np.int64)
        assert_bits(launch(tables, same_q, pair_t, 0, 0, same_q.shape[0]),
                    tc.expected_features(oracle, case, same_q, pair_t), ("one query", q))


def test_records_rebuilt_on_a_live_table(oracle):
    """One live truth table, (number_of_truth_titles, space code) changing under it: the records are rebuilt for every
    change, dropped and built again with the option -- never stale.  1 and a value above every word count; space code 2
    moves every word boundary."""
    tables = Tables(tc.forms_case())
    case = tables.case
    k, q_first = 17, 0
    rows = tc.forms_rows(case, k, q_first)
    pair_q, pair_t = tc.pairs_of_rows(rows, q_first)
    a, b = 1, int(case.t_counts.max()) + 1
    memo = {}

    def check(n_truth, space, step):
        if (n_truth, space) not in memo:
            memo[n_truth, space] = tc.expected_features(oracle, case, pair_q, pair_t, n_truth, space)
        assert_bits(launch(tables, None, rows, q_first, k, rows.size, n_truth, space), memo[n_truth, space], step)

    for step, (n_truth, space) in enumerate(((a, 1), (b, 1), (a, 1), (a, 2))):
        check(n_truth, space, step)
    assert not np.array_equal(memo[a, 1], memo[b, 1]) and not np.array_equal(memo[a, 1], memo[a, 2])
    tables.truth.option("truth_records", 0)
    check(a, 2, "off")
    check(b, 1, "off, changed")
    tables.truth.option("truth_records", 1)
    check(b, 1, "on again")
    check(a, 2, "on again, changed")


@pytest.mark.parametrize("stride", [16, 64, 300])
def test_strides_other_than_255(oracle, stride):
    """Tables whose rows are 16, 64 and 300 bytes apart, lengths up to min(stride, 255)."""
    case = tc.make_case(400, 300, seed=3000 + stride, stride=stride)
    assert case.q_enc.shape[1] == stride and int(case.q_len.max()) == min(stride, 255) == int(case.t_len.max())
    tables = Tables(case)
    for k in (3, 17):
        n_queries = 150
        q_first = case.n_q - n_queries
        rows = tc.make_rows(case, q_first, n_queries, k, seed=stride + k)
        pair_q, pair_t = tc.pairs_of_rows(rows, q_first)
        expected = tc.expected_features(oracle, case, pair_q, pair_t)
        for records in (1, 0):
            tables.truth.option("truth_records", records)
            assert_bits(launch(tables, None, rows, q_first, k, rows.size), expected, (stride, k, records))


def test_more_units_than_the_grid_holds(oracle):
    """One rows-form launch of 40,000 queries x k = 16 on the hostile tables: 40,000 units for a grid capped at 1,280
    workgroups x 4 waves that take 2 units per pop -- every wave goes back to the queue about four times.  ALL 640,000
    pairs are compared with the oracle.  Measured on the CPU alone, on 8 cores with 16 OpenMP threads:
    oracle.construct_features takes 6 to 7 s for the 640,000 pairs, generating the tables 1.9 s and the rows 0.5 s."""
    case = tc.grid_case()
    tables = Tables(case)
    rows = tc.make_rows(case, 0, tc.GRID_QUERIES, tc.GRID_K, seed=5)
    pair_q, pair_t = tc.pairs_of_rows(rows, 0)
    units, _ = tc.units_of(rows.size, tc.GRID_K)
    assert units == 40000
    got = launch(tables, None, rows, 0, tc.GRID_K, rows.size)
    expected = tc.expected_features(oracle, case, pair_q, pair_t)
    assert_bits(got, expected, "grid")
    literal = tc.literal_pairs(case, pair_q, pair_t)[0]
    assert literal.sum() > 100000 and (~literal).sum() > 100000


def test_two_streams_hostile_titles(oracle, tables):
    """Launches on two streams over one truth table, enqueued back to back as in
    test_overlapping_launches_on_two_streams_share_one_truth_table: every buffer is allocated and filled first, then six
    launches follow each other with nothing between them (no allocation, no fill, no synchronisation), each with a queue head
    of its own, and both streams are waited for at the end.  k = 17: the units that cover two queries meet launches that
    overlap.  1,400 queries (23,800 hostile pairs, 2,380 units) per launch keep a kernel resident while the next arrives."""
    from doppel_speller_amd import _lib
    case = tables.case
    tables.truth.option("truth_records", 1)
    k, n_queries = 17, 1400
    firsts = (0, case.n_q - n_queries)
    all_rows = [tc.make_rows(case, q_first, n_queries, k, seed=40 + q_first) for q_first in firsts]
    assert all(tc.straddling_units(tc.pairs_of_rows(rows, q_first)[0], k) >= n_queries // 2
               for rows, q_first in zip(all_rows, firsts))
    # the records exist before the overlapping launches (their first build synchronises its stream)
    launch(tables, None, all_rows[0][:1], 0, k, k)
    streams = []
    for _ in all_rows:
        stream = ctypes.c_void_p()
        _lib.check(_lib.lib().ds_stream_create(0, ctypes.byref(stream)), "ds_stream_create")
        streams.append(stream)
    d_rows = [_lib.DeviceArray.from_host(rows) for rows in all_rows]
    outs = [[filled_output(rows.size) for rows in all_rows] for repeat in range(3)]
    for repeat in range(3):   # several rounds: the launches of one round overlap, the heads rotate
        for which, (stream, rows, d, q_first) in enumerate(zip(streams, all_rows, d_rows, firsts)):
            enqueue(tables, None, d, q_first, k, rows.size, tc.N_TRUTH, tc.SPACE, outs[repeat][which], stream)
    for stream in streams:
        _lib.check(_lib.lib().ds_stream_sync(stream, 0), "sync")
    for which, (rows, q_first) in enumerate(zip(all_rows, firsts)):
        pair_q, pair_t = tc.pairs_of_rows(rows, q_first)
        expected = tc.expected_features(oracle, case, pair_q, pair_t)
        for repeat in range(3):
            assert_bits(outs[repeat][which].to_host().view(np.uint32), expected, (q_first, repeat))
    for stream in streams:
        _lib.lib().ds_stream_destroy(stream, 0)
