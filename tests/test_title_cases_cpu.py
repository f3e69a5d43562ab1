"""What tests/title_cases.py generates, checked from the inputs alone: the committed seeds reach every path the GPU tests
of the features and close-match launch forms are named for (tests/test_gpu_features_forms.py,
tests/test_gpu_close_matches_forms.py).  A softer generator fails HERE instead of the GPU tests quietly testing less.
The minimums are about half of what the committed seeds give (printed by -s), never more than the case can hold.
The oracle runs over the case once: the expected values exist for every pair."""
import numpy as np
import pytest

import title_cases as tc


@pytest.fixture(scope="module")
def case():
    return tc.forms_case()


def test_pairs_per_unit_restated():
    assert [tc.pairs_per_unit(k) for k in tc.FEATURE_KS] == [1, 2, 3, 7, 15, 16, 10, 10, 12, 16, 10, 10]
    assert tc.pairs_per_unit(0) == 8 and tc.pairs_per_unit(48) == 16 and tc.pairs_per_unit(50) == 10
    # the restatement follows the kernel's source
    import os
    source = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "doppel-speller_amd", "csrc",
                               "ds_features.hip")).read()
    body = source[source.index("static int32_t pairs_per_unit(int32_t k)"):]
    body = " ".join(body[:body.index("}\n\n")].split())
    assert "if (k <= 0) return 8; if (k <= 16) return k; for (int32_t d = 16; d >= 8; --d) if (k % d == 0) return d; return 10;" in body


def test_tables_hold_every_edge(case):
    for enc, lengths, large in ((case.q_enc, case.q_len, case.q_large), (case.t_enc, case.t_len, case.t_large)):
        assert set(tc.EDGE_LENGTHS) <= set(lengths.tolist())
        for length in tc.EDGE_LENGTHS:                      # every edge length with and without a code >= 64
            if length:
                assert large[lengths == length].any() and (~large[lengths == length]).any(), length
        words = tc.word_counts(enc, lengths)
        inside = np.arange(enc.shape[1])[None, :] < lengths[:, None]
        spaces = ((enc == tc.SPACE) & inside).sum(axis=1)
        assert (lengths == 0).sum() >= 10
        assert ((lengths > 0) & (spaces == lengths)).sum() >= 10                      # nothing but spaces
        first = enc[:, 0] == tc.SPACE
        last = enc[np.arange(enc.shape[0]), np.maximum(lengths.astype(np.int64) - 1, 0)] == tc.SPACE
        assert ((lengths > 2) & first & (words > 0)).sum() >= 20                      # leading spaces
        assert ((lengths > 2) & last & (words > 0)).sum() >= 20                       # trailing spaces
        doubled = ((enc[:, 1:] == tc.SPACE) & (enc[:, :-1] == tc.SPACE) & inside[:, 1:]).any(axis=1)
        assert (doubled & (words > 1)).sum() >= 20                                    # repeated spaces inside
        assert (words == 128).sum() >= 2                                              # 128 one-letter words
    # empty queries next to 255-character ones
    lq = case.q_len.astype(np.int64)
    assert (((lq[:-1] == 0) & (lq[1:] == 255)) | ((lq[:-1] == 255) & (lq[1:] == 0))).sum() >= 10
    # truth titles of 1, 15, 16 and more words; a word longer than 64 characters
    t_inside = np.arange(case.stride)[None, :] < case.t_len[:, None]
    truth_words = ((case.t_enc == tc.SPACE) & t_inside).sum(axis=1) + 1               # spaces + 1, as the kernel counts
    for wanted in (1, 15, 16, 40, 128):
        assert (truth_words == wanted).sum() >= 2, wanted
    assert (truth_words > 15).sum() >= 50
    longest = np.zeros(case.n_t, dtype=np.int64)
    run = np.zeros(case.n_t, dtype=np.int64)
    for column in range(case.stride):
        is_char = (case.t_enc[:, column] != tc.SPACE) & t_inside[:, column]
        run = np.where(is_char, run + 1, 0)
        longest = np.maximum(longest, run)
    assert ((longest > 64) & ~case.t_large).sum() >= 20 and (longest == 65).sum() >= 1 and (longest == 64).sum() >= 1
    # word counts of 0, 1, n_truth and above it; whole rows of zeros
    for value in (0, 1, tc.N_TRUTH):
        assert (case.t_counts == value).sum() >= 500, value
    assert (case.t_counts > tc.N_TRUTH).sum() >= 1000 and case.t_counts.max() == 5 * tc.N_TRUTH
    assert (case.t_counts == 0).all(axis=1).sum() >= 50
    assert len(case.derived) >= 200 and (case.t_source >= 0).sum() >= 300


@pytest.mark.parametrize("k", tc.FEATURE_KS)
def test_rows_reach_every_path(case, k):
    n_queries = tc.forms_queries(k)
    for q_first in (0, case.n_q - n_queries):
        rows = tc.forms_rows(case, k, q_first)
        assert rows.shape == (n_queries, k) and rows.dtype == np.int32
        pair_q, pair_t = tc.pairs_of_rows(rows, q_first)
        assert pair_q[-1] == q_first + n_queries - 1 and (q_first == 0 or pair_q[-1] == case.n_q - 1)
        n = pair_q.shape[0]
        valid = tc.valid_pairs(case, pair_q, pair_t)
        literal, too_long, wide_pattern, big_code = tc.literal_pairs(case, pair_q, pair_t)
        small = ~(case.q_large[pair_q] | case.t_large[np.where(valid, pair_t, 0)])
        lt = case.t_len[np.where(valid, pair_t, 0)].astype(np.int64)
        figures = dict(k=k, q_first=q_first, pairs=n, outside=int((~valid).sum()), too_long=int(too_long.sum()),
                       wide_pattern=int(wide_pattern.sum()), big_code=int(big_code.sum()),
                       bit_parallel=int((valid & ~literal).sum()),
                       literal_then_not=tc.mixed_runs(literal, valid, k), alphabet_flips=tc.mixed_runs(small, valid, k),
                       empty_then_full=tc.mixed_runs(lt == 0, valid & ((lt == 0) | (lt == 255)), k),
                       straddling=tc.straddling_units(pair_q, k), units=tc.units_of(n, k))
        print(figures)
        # rows outside the table: -1, n_t, INT32_MAX, whole queries of -1, the first and the last slot of a row
        assert figures["outside"] >= n // 20
        assert (rows == -1).all(axis=1).sum() >= n_queries // 40 and (rows[:, 0] == -1).sum() >= n_queries // 12
        assert (rows[:, k - 1] == case.n_t).sum() >= n_queries // 15
        if k >= 3:
            assert (rows == tc.INT32_MAX).sum() >= 1 and (rows == case.n_t).sum() >= 1
        # the three reasons for the literal path, and the bit-parallel path
        assert figures["too_long"] >= n // 50 and figures["wide_pattern"] >= n // 100 and figures["big_code"] >= n // 10
        assert figures["bit_parallel"] >= n // 5
        if k >= 2:      # the path changes inside one query's run, the query staying staged
            enough = n_queries // 8
            assert figures["literal_then_not"] >= enough and figures["alphabet_flips"] >= enough
            assert figures["empty_then_full"] >= n_queries // 16
            repeated = (rows[:, 1:] == rows[:, :-1]) & (rows[:, 1:] >= 0) & (rows[:, 1:] < case.n_t)
            assert repeated.any(axis=1).sum() >= n_queries // 16                # the same truth row twice in a row
            assert ((rows[1:, 0] == rows[:-1, k - 1]) & (rows[1:, 0] >= 0)).sum() >= n_queries // 32  # and across queries
        # units that cover two queries: exactly where the unit does not divide k
        if k in (17, 23, 127):
            assert figures["straddling"] >= n_queries // 2
            assert n % figures["units"][1] != 0                                 # and the last unit is partial
        else:
            assert figures["straddling"] == 0 and k % figures["units"][1] == 0


def test_grid_case_needs_several_pops_per_wave():
    units, per_unit = tc.units_of(tc.GRID_QUERIES * tc.GRID_K, tc.GRID_K)
    assert per_unit == 16 and units == 40000 and units >= 3 * 1280 * 4 * 2      # grid cap x waves x kFeatPop


def test_oracle_defines_every_valid_pair(case, oracle):
    """oracle.construct_features over one whole launch of the case: NaN exactly where construct_features defines it (the
    words a truth title does not have; the rank of a word whose count is 0, inf - inf), finite or infinite elsewhere."""
    k = 17
    rows = tc.forms_rows(case, k, 0)
    pair_q, pair_t = tc.pairs_of_rows(rows, 0)
    valid = tc.valid_pairs(case, pair_q, pair_t)
    for n_truth, space in ((tc.N_TRUTH, tc.SPACE), (1, 2)):
        bits = tc.expected_features(oracle, case, pair_q, pair_t, n_truth, space)
        assert (bits[~valid] == tc.NAN_BITS).all()
        features = bits.view(np.float32)[valid]
        t = pair_t[valid]
        inside = np.arange(case.stride)[None, :] < case.t_len[t][:, None]
        n_words = np.minimum(((case.t_enc[t] == space) & inside).sum(axis=1) + 1, tc.WORDS)
        beyond = np.arange(tc.WORDS)[None, :] >= n_words[:, None]
        assert not np.isnan(features[:, :6]).any()
        for block in range(3):                               # best ratios, word lengths, idf_s
            assert np.array_equal(np.isnan(features[:, 6 + 15 * block:21 + 15 * block]), beyond), block
        idf = features[:, 36:51]
        assert np.array_equal(np.isnan(features[:, 51:66]), beyond | np.isposinf(idf))
        assert np.isposinf(idf).any() and (idf < 0).any() and (idf == 0).any()
        assert np.array_equal(features[:, 0], case.q_len[pair_q[valid]].astype(np.float32))
        assert features[:, 4].max() <= 100 and (features[:, 4] >= 90).sum() >= 5


def test_close_case_reaches_every_path(oracle):
    from doppel_speller_amd.feature_engineering import SORT_KEY
    case = tc.close_case()
    seen_ties = 0
    for k in tc.CLOSE_KS:
        n_queries = tc.close_queries(k)
        for q_first in (0, case.n_q - n_queries):
            rows = tc.make_rows(case, q_first, n_queries, k, seed=2000 + k)
            pair_q, pair_t = tc.pairs_of_rows(rows, q_first)
            valid = tc.valid_pairs(case, pair_q, pair_t)
            assert (~valid).sum() >= pair_q.shape[0] // 20
            for threshold in tc.CLOSE_THRESHOLDS:
                ratios = tc.expected_ratios(oracle, case, pair_q, pair_t, threshold, SORT_KEY).reshape(rows.shape)
                assert ratios.max() <= 100 and (ratios.reshape(-1)[~valid] == 0).all()
                best = tc.best_from_ratios(ratios, rows, threshold)
                top = ratios.max(axis=1)
                ties = int(((top > threshold) & ((ratios == top[:, None]).sum(axis=1) > 1)).sum())
                print(dict(k=k, q_first=q_first, threshold=threshold, above=int((ratios > threshold).sum()),
                           matched=int((best >= 0).sum()), ties=ties))
                assert ((best >= 0) & (best < case.n_t)).sum() == (best >= 0).sum()    # never a row outside the table
                if threshold == 100:
                    assert (best == -1).all()
                elif q_first == 0:
                    assert (best >= 0).sum() >= 3
                    seen_ties += ties
                    if k >= 10 and threshold <= 94:
                        assert ties >= 3                      # two equal best ratios: no match
    assert seen_ties >= 100
    # the special rows, every one against every one: two empty titles, spaces only on either side, 128 words on both
    q_special = tc.special_rows(case.q_enc, case.q_len, case.q_large)
    t_special = tc.special_rows(case.t_enc, case.t_len, case.t_large)
    assert q_special.shape[0] >= 40 and t_special.shape[0] >= 40
    q_words, t_words = tc.word_counts(case.q_enc, case.q_len)[q_special], tc.word_counts(case.t_enc, case.t_len)[t_special]
    assert (case.q_len[q_special] == 0).sum() >= 2 and (case.t_len[t_special] == 0).sum() >= 2
    assert (q_words == 128).sum() >= 1 and (t_words == 128).sum() >= 1
    assert ((q_words == 0) & (case.q_len[q_special] > 0)).sum() >= 4 and ((t_words == 0) & (case.t_len[t_special] > 0)).sum() >= 4
    assert case.q_large[q_special].sum() >= 10 and case.t_large[t_special].sum() >= 10
    pair_q, pair_t = np.repeat(q_special, t_special.shape[0]), np.tile(t_special, q_special.shape[0])
    ratios = tc.expected_ratios(oracle, case, pair_q, pair_t, 94, SORT_KEY)
    both_empty = (case.q_len[pair_q] == 0) & (case.t_len[pair_t] == 0)
    assert both_empty.sum() >= 4 and (ratios[both_empty] == 100).all()      # the oracle's reading of 0/0
    # one launch past the 32,768 pairs of one pass of the close-ratio kernel's grid
    assert tc.CLOSE_PASS_QUERIES * 10 > 8192 * 4 and tc.CLOSE_PASS_QUERIES <= case.n_q
