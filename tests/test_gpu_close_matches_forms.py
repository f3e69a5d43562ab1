"""ds_close_matches_device (ds_close_ratio_kernel + ds_close_best_kernel) in the rows form on hostile titles
(tests/title_cases.py): every ratio against oracle.close_ratios, 0 for a candidate outside the table, the best row against
the restatement of predict.py:172-176 -- exact, for every pair.  Both output buffers are filled with a value the kernels
never write in front of every launch.  tests/test_title_cases_cpu.py pins what the case holds."""
import ctypes

import numpy as np
import pytest

import title_cases as tc

pytestmark = pytest.mark.gpu

RATIO_SENTINEL = 0xee                    # 238: no ratio (0..100)
BEST_SENTINEL = -0x11111112              # int32 0xeeeeeeee


class Tables:
    def __init__(self, case):
        from doppel_speller_amd import _lib
        from doppel_speller_amd.feature_engineering import SORT_KEY, TitleTable
        self.case = case
        self.queries = TitleTable(case.q_enc, case.q_len)
        self.truth = TitleTable(case.t_enc, case.t_len, case.t_counts)
        self.sort_key = SORT_KEY
        self.d_sort_key = _lib.DeviceArray.from_host(SORT_KEY)


@pytest.fixture(scope="module")
def tables():
    return Tables(tc.close_case())


def close_matches(tables, rows, q_first, threshold, with_best=True, space=tc.SPACE):
    """One ds_close_matches_device launch -> (ratios uint8[Q, k], best int32[Q] or None)."""
    from doppel_speller_amd import _lib
    lib = _lib.lib()
    n_queries, k = rows.shape
    d_rows = _lib.DeviceArray.from_host(np.ascontiguousarray(rows, dtype=np.int32))
    d_ratios = _lib.DeviceArray((n_queries, k), np.uint8)
    d_best = _lib.DeviceArray((n_queries,), np.int32)
    _lib.check(lib.ds_memset(d_ratios.ptr, RATIO_SENTINEL, d_ratios.nbytes, 0), "ds_memset")
    _lib.check(lib.ds_memset(d_best.ptr, RATIO_SENTINEL, d_best.nbytes, 0), "ds_memset")
    _lib.check(lib.ds_stream_sync(None, 0), "sync")
    _lib.check(lib.ds_close_matches_device(tables.queries.handle, tables.truth.handle, d_rows.ptr, q_first, k, n_queries,
                                           space, tables.d_sort_key.ptr, threshold, d_ratios.ptr,
                                           d_best.ptr if with_best else ctypes.c_void_p(0), ctypes.c_void_p(0)),
               "ds_close_matches_device")
    _lib.check(lib.ds_stream_sync(None, 0), "sync")
    best = d_best.to_host()
    if not with_best:
        assert (best == BEST_SENTINEL).all()                 # d_best_row = NULL: ratios only, nothing else written
        best = None
    return d_ratios.to_host(), best


def check(oracle, tables, rows, q_first, threshold, what):
    pair_q, pair_t = tc.pairs_of_rows(rows, q_first)
    expected = tc.expected_ratios(oracle, tables.case, pair_q, pair_t, threshold, tables.sort_key).reshape(rows.shape)
    ratios, best = close_matches(tables, rows, q_first, threshold)
    wrong = np.nonzero(ratios != expected)
    assert wrong[0].shape[0] == 0, (what, wrong[0].shape[0], wrong[0][:5], wrong[1][:5], ratios[wrong][:5], expected[wrong][:5],
                                    pair_q.reshape(rows.shape)[wrong][:5], rows[wrong][:5])
    expected_best = tc.best_from_ratios(expected, rows, threshold)
    assert np.array_equal(best, expected_best), (what, np.nonzero(best != expected_best)[0][:5])
    return expected, expected_best


@pytest.mark.parametrize("threshold", tc.CLOSE_THRESHOLDS)
@pytest.mark.parametrize("k", tc.CLOSE_KS)
def test_rows_form(oracle, tables, k, threshold):
    """q_first = 0 and the last queries of the table; rows with -1 / n_t / INT32_MAX entries, the same candidate twice in a
    row (two equal best ratios: no match); the pre-filter moves with the threshold, nothing matches at 100."""
    case = tables.case
    n_queries = tc.close_queries(k)
    for q_first in (0, case.n_q - n_queries):
        rows = tc.make_rows(case, q_first, n_queries, k, seed=2000 + k)
        expected, best = check(oracle, tables, rows, q_first, threshold, (k, threshold, q_first))
        outside = (rows < 0) | (rows >= case.n_t)
        assert outside.sum() >= rows.size // 20 and (expected[outside] == 0).all()
        assert ((best >= 0) & (best < case.n_t)).sum() == (best >= 0).sum()
        if threshold == 100:
            assert (best == -1).all()


@pytest.mark.parametrize("threshold", [0, 94])
def test_special_titles_every_one_against_every_one(oracle, tables, threshold):
    """Empty and space-only titles on either side (two empty titles: 100, the oracle's reading of the reference's 0/0),
    128 one-letter words on both sides (the capacity of the token table), short titles with a code >= 64 (the diagonal DP)."""
    case = tables.case
    q_special = tc.special_rows(case.q_enc, case.q_len, case.q_large)
    t_special = tc.special_rows(case.t_enc, case.t_len, case.t_large)
    # the rows form reads consecutive query rows: a query table of the special rows alone
    special = tc.Case(case.q_enc[q_special], case.q_len[q_special], case.t_enc, case.t_len, case.t_counts, case.t_source)
    small = Tables(special)
    rows = np.tile(t_special, (q_special.shape[0], 1)).astype(np.int32)
    expected, _ = check(oracle, small, rows, 0, threshold, ("special", threshold))
    both_empty = (special.q_len[:, None] == 0) & (case.t_len[t_special][None, :] == 0)
    assert both_empty.sum() >= 4 and (expected[both_empty] == 100).all()


def test_more_pairs_than_one_pass_of_the_grid(oracle, tables):
    """5,000 queries x k = 10 = 50,000 pairs, and 400 x k = 100 = 40,000: the grid is capped at 8,192 workgroups x 4 waves
    = 32,768 pairs per pass, the grid-stride loop takes a second one.  Every ratio is compared."""
    case = tables.case
    for k, n_queries in ((10, tc.CLOSE_PASS_QUERIES), (100, 400)):
        assert n_queries * k > 8192 * 4
        q_first = case.n_q - n_queries
        rows = tc.make_rows(case, q_first, n_queries, k, seed=k)
        expected, best = check(oracle, tables, rows, q_first, 94, ("two passes", k))
        second_pass = expected.reshape(-1)[8192 * 4:]
        assert (second_pass > 0).sum() >= 200 and (second_pass > 94).sum() >= (10 if k == 10 else 1) and (best >= 0).sum() >= 5


def test_ratios_only(oracle, tables):
    """d_best_row = NULL: the ratios are written, the best rows are not touched."""
    case = tables.case
    rows = tc.make_rows(case, 0, 500, 10, seed=2010)
    pair_q, pair_t = tc.pairs_of_rows(rows, 0)
    ratios, best = close_matches(tables, rows, 0, 94, with_best=False)
    assert best is None
    assert np.array_equal(ratios, tc.expected_ratios(oracle, case, pair_q, pair_t, 94, tables.sort_key).reshape(rows.shape))
