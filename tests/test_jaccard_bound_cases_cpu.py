"""jaccard_bound_cases.py proved from its inputs alone, in float64 NumPy and without a GPU: every case has the tiles, the
signature bits, the skipped columns under the bound with and without the band edge, and the rows on either side of the cut
that test_gpu_jaccard_bound.py relies on."""
import functools

import numpy as np
import pytest

import jaccard_bound_cases as bc
import jaccard_cases as jc

decisive = functools.lru_cache(maxsize=None)(bc.decisive_problem)
high_bits = functools.lru_cache(maxsize=None)(bc.high_bits_problem)
padding = functools.lru_cache(maxsize=None)(bc.padding_problem)
capped = functools.lru_cache(maxsize=None)(bc.capped_table_problem)


def _three_tiles_and_a_row(case, geometry):
    tile_rows = jc.GEOMETRY[geometry]["tile_rows"]
    assert case["sums32"].shape[0] == 3 * tile_rows + 1 and jc.tiles_of(case, geometry) == 4 == case["tiles"]
    # no row's sums32 lies below the total of its columns by more than ds_index_create allows (1e-4): the fast kernel serves it
    totals = np.zeros(case["sums32"].shape[0])
    columns = np.repeat(np.arange(case["rowptr"].shape[0] - 1), np.diff(case["rowptr"]))
    np.add.at(totals, case["truth_idx"], case["idf32"][columns].astype(np.float64))
    assert np.all(case["sums32"].astype(np.float64) >= totals * (1.0 - 1e-5))
    assert np.unique(case["sums32"]).shape[0] > case["sums32"].shape[0] * 0.99       # twins would need every column AND sums32 equal


def _positive_rows_of_tile(case, q, geometry, tile):
    tile_rows = jc.GEOMETRY[geometry]["tile_rows"]
    scores, _ = jc.jaccard_rows(case, q)
    members = jc.internal_order(case)[tile * tile_rows:(tile + 1) * tile_rows]
    return np.sort(members[scores[members] > 0])


@pytest.mark.parametrize("geometry", jc.GEOMETRIES)
def test_decisive_column(geometry):
    case = decisive(geometry)
    _three_tiles_and_a_row(case, geometry)
    g = jc.GEOMETRY[geometry]
    bits = bc.signature_bits(case)
    columns, masses = bc.prefix_masses(case, 0)
    maxint = float(case["q_maxint"][0])
    assert columns.tolist() == [0, 1, 2, 3, 4] and all(int(c) in bits for c in columns)
    assert int(columns[2]) == case["decisive_column"]
    ranges = jc.tile_ranges(case, geometry)
    assert jc.start_tile(case, 0, ranges) == 2
    # the start tile's rows with a positive score are the 560 full rows: whatever threshold the kernel forms first -- the
    # k-th best of one or two samples per thread, or of the rows themselves once the tile is scanned -- is a value of theirs.
    # 560 rows lie in at least 560 / (tile_rows / threads) >= 10 threads' shares of the tile; they fit the candidate buffer
    # below its selection trigger; and they are at least max(k, 16) rows, so a scan without a threshold ends in a selection
    full = case["full"]
    assert np.array_equal(_positive_rows_of_tile(case, 0, geometry, 2), full)
    assert full.shape[0] * g["threads"] >= 10 * g["tile_rows"] and 100 <= full.shape[0] <= jc.select_trigger(geometry) - 64
    floor = bc.first_cut_floor(case, 0, geometry, full) - 1e-3         # (+ the kernel's own margins: 2e-6 and the rounding)
    scores, values = jc.jaccard_rows(case, 0)
    for k in bc.DECISIVE_K:
        final, below = bc.kth_value(case, 0, k)
        assert final - below > 1e-5                                      # no tie at the cut
        assert floor < final
        for cut in np.linspace(floor, final, 50):
            assert bc.skipped_count(case, 0, cut, True, bits) == 3 and bc.skipped_count(case, 0, cut, False, bits) == 2
        # under the FINAL cut the decisive prefix lies between the two bounds with 5 % of maxint to either side, and the
        # next prefix 5 % above the new one: exactly one more column
        assert bc.pre_bound(case, 0, final, False) + 0.05 * maxint <= masses[2] <= bc.pre_bound(case, 0, final) - 0.05 * maxint
        assert masses[3] >= bc.pre_bound(case, 0, final) + 0.05 * maxint
        assert bc.pre_bound(case, 0, floor) - masses[2] >= 0.05 * maxint      # ... and under the first cut already
        best = np.argsort(-values, kind="stable")[:k]
        assert np.isin(best, case["completed"]).sum() >= 1                # (b) rows end among the k best
        # (c): in tile 0, which the band keeps (its largest sums32 reaches cut * maxint), below the band edge themselves
        assert ranges[1][0] >= final * maxint and np.all(case["sums32"][case["below_band"]] < final * maxint * (1.0 - 1e-5))
        assert np.all(case["sums32"][case["below_band"]] > 0.95 * final * maxint)
    # (a): skipped columns only; sums32 within 2 % of their total, i.e. as close to the cut as such rows get
    assert np.all(scores[case["only_skipped"]] == scores[case["only_skipped"]][0])
    assert abs(float(scores[case["only_skipped"]][0]) - masses[2]) < 1e-5
    assert np.all(values[case["only_skipped"]] > masses[2] / (maxint * 1.02))
    # (b): the decisive column plus ONE essential column, across the edge of tiles 0 and 1
    assert set(jc.columns_of_rows(case, case["completed"][:3])[int(case["completed"][0])][:2]) == {2, 4}
    tile_of = np.empty(case["sums32"].shape[0], dtype=np.int64)
    tile_of[jc.internal_order(case)] = np.arange(case["sums32"].shape[0]) // g["tile_rows"]
    assert set(tile_of[case["completed"]].tolist()) == {0, 1} and set(tile_of[case["below_band"]].tolist()) == {0}


@pytest.mark.parametrize("geometry", jc.GEOMETRIES)
def test_membership_bits_8_to_15(geometry):
    case = high_bits(geometry)
    _three_tiles_and_a_row(case, geometry)
    bits = bc.signature_bits(case)
    assert [bits[g] for g in range(16)] == list(range(16))               # G_g owns signature bit g
    assert jc.start_tile(case, 0, jc.tile_ranges(case, geometry)) == 2
    full = case["full"]
    positive = _positive_rows_of_tile(case, 0, geometry, 2)
    scores, values = jc.jaccard_rows(case, 0)
    # the start tile: the full rows and the ballast, whose values are two orders below (no threshold comes from them as long
    # as k = 10 threads' shares hold a full row: 560 rows lie in at least 10)
    assert np.all(np.isin(full, positive)) and values[np.setdiff1d(positive, full)].max() < 0.02
    g = jc.GEOMETRY[geometry]
    assert full.shape[0] * g["threads"] >= 10 * g["tile_rows"]
    floor = bc.first_cut_floor(case, 0, geometry, full) - 1e-3
    final, below = bc.kth_value(case, 0, 10)
    assert final - below > 1e-5 and floor < final
    columns, masses = bc.prefix_masses(case, 0)
    assert columns[:16].tolist() == list(range(16))
    for cut in np.linspace(floor, final, 50):                             # exactly G0..G15 are skipped
        assert bc.skipped_count(case, 0, cut, True, bits) == 16
    maxint = float(case["q_maxint"][0])
    best = np.argsort(-values, kind="stable")[:10]
    assert np.isin(best, case["high"]).sum() >= 3 and np.isin(best, case["low"]).sum() >= 3
    assert values[case["without"]].max() < floor - 0.1                    # the other side of every cut
    # `high` and `without` differ only in G8..G15 (sums32 within 0.001 of each other), and those columns decide: the
    # essential score alone stays below the weakest gate, with them it passes the strongest
    assert np.allclose(np.sort(case["sums32"][case["without"]]) - np.sort(case["sums32"][case["high"]]), 0.001, atol=1e-5)
    essential = float(case["idf32"][17])
    assert np.all(scores[case["without"]] == np.float32(essential))
    assert essential < bc.pre_bound(case, 0, floor) - 0.1 * maxint
    assert float(scores[case["high"]][0]) >= final * maxint and float(scores[case["low"]][0]) >= final * maxint
    own = jc.columns_of_rows(case, np.concatenate((case["high"][:1], case["low"][:1])))
    assert own[int(case["high"][0])][:9] == tuple(range(8, 16)) + (17,) and own[int(case["low"][0])][:9] == tuple(range(8)) + (17,)


def test_capped_table_trap():
    case = capped()
    assert case["sums32"].shape[0] == 24581 and case["rowptr"].shape[0] - 1 == 3 and case["k"] == 1
    assert jc.tiles_of(case, "narrow") == 3 and jc.tiles_of(case, "wide") == 1
    held = np.zeros(24581, dtype=np.int64)                                  # no twins: equal sums32 only with other columns
    np.add.at(held, case["truth_idx"], 1 << np.repeat(np.arange(3), np.diff(case["rowptr"])))
    assert np.unique(held * 100.0 + case["sums32"].astype(np.float64)).shape[0] == 24581 and held.min() >= 1
    bits = bc.signature_bits(case)
    assert set(bits) == {0, 1, 2}
    columns, masses = bc.prefix_masses(case, 0)
    maxint = float(case["q_maxint"][0])
    assert columns.tolist() == [0, 1, 2] and masses[1] > 0.6 * maxint         # A, B: more than half of the query's mass
    ranges = jc.tile_ranges(case, "narrow")
    assert jc.start_tile(case, 0, ranges) == 1                                # tile 2 lies ABOVE the start tile
    scores, values = jc.jaccard_rows(case, 0)
    winner = int(case["winner"][0])
    assert int(np.argmax(values)) == winner and np.sort(values)[-1] - np.sort(values)[-2] > 0.05
    order = jc.internal_order(case)
    assert winner in order[2 * 12288:].tolist() and float(case["sums32"][winner]) == float(ranges[0][2])
    # the start tile: k = 1, so the first cut is the best sample, the best score of the tile over the tile's largest sums32
    # (+ maxint - score); the rows whose own value reaches it are the 300 {B, C} rows: at least max(k, 16), so the tile's
    # scan ends in a selection, and fewer than the selection trigger keeps.  The cut after it is their best value.
    start_rows = order[12288:2 * 12288]
    best_score = float(scores[start_rows].max())
    first_cut = best_score / (float(ranges[1][1]) + (maxint - best_score))
    reach = np.sort(start_rows[values[start_rows] >= first_cut - 1e-3])
    assert np.array_equal(reach, case["bc"]) and 16 <= reach.shape[0] <= jc.select_trigger("narrow") - 64
    cut_lo = float(values[case["bc"]].max()) - 1e-3                           # (- the kernel's margins, 2e-6 and roundings)
    cut_hi = float(values[winner])
    # under every cut between the start tile's selection and the final one A and B are skipped, C is not ...
    for cut in np.linspace(cut_lo, cut_hi, 20):
        assert bc.skipped_count(case, 0, cut, True, bits) == 2
    # ... tile 2 stays inside the band (tile_sums_min * cut <= maxint) ...
    assert float(ranges[0][2]) * cut_hi <= maxint * 1.00001
    # ... and the winner's C posting meets the tile's gate, coef * (the tile's smallest sums32 + maxint), never below pre:
    # with the true mass of A and B it passes, with an entry capped at 32,000 fixed-point units it does not
    essential = float(case["idf32"][2])
    capped_mass = bc.CAPPED_UNITS / bc.FIXED_ONE * maxint
    assert capped_mass < masses[1]
    for cut in np.linspace(cut_lo, cut_hi, 20):
        gate = max(cut / (1.0 + cut) * (float(ranges[0][2]) + maxint), bc.pre_bound(case, 0, cut))
        assert essential + masses[1] >= gate * (1.0 - 1e-6) and essential + capped_mass < gate - 0.05 * maxint
    # the sparse tile holds nothing else of the query's essential column
    tile2 = order[2 * 12288:]
    assert (held[tile2] & 4).sum() == 4 and held[winner] == 7


@pytest.mark.parametrize("geometry", jc.GEOMETRIES)
def test_padding_and_no_threshold(geometry):
    case = padding(geometry)
    _three_tiles_and_a_row(case, geometry)
    tile_rows = jc.GEOMETRY[geometry]["tile_rows"]
    tile_of = np.empty(case["sums32"].shape[0], dtype=np.int64)
    tile_of[jc.internal_order(case)] = np.arange(case["sums32"].shape[0]) // tile_rows
    for q, n in enumerate(bc.PADDING_LISTS):
        rows = case["p%d" % n]
        per_tile = np.bincount(tile_of[rows], minlength=4).tolist()
        assert per_tile == [n, n, n, 1 if n == 1 else 0]                 # n postings per tile; one list in the partial tile
        assert n % 4 != 0                                                # every (column, tile) list ends in padding
        k = case["k_of_query"][q]
        assert k == rows.shape[0]
        _, values = jc.jaccard_rows(case, q)
        best = np.argsort(-values, kind="stable")[:k]
        assert np.array_equal(np.sort(best), rows)                       # the answer is exactly the rows next to the padding
        assert values[rows].min() > 0.45 and np.delete(values, rows).max() < 0.22
        # under the final cut S is skipped and Pn essential
        final, _ = bc.kth_value(case, q, k)
        assert bc.skipped_count(case, q, final) == 1 and bc.prefix_masses(case, q)[0][0] == 0
    for q, holders in ((4, 6), (5, 9)):                                  # fewer than k = 10 positive rows: no threshold
        scores, _ = jc.jaccard_rows(case, q)
        assert int(np.sum(scores > 0)) == holders < case["k_of_query"][q] == 10
        assert bc.pre_bound(case, q, 0.0) == 0.0 and bc.skipped_count(case, q, 0.0) == 0
