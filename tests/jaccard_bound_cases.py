"""Inputs for the Jaccard top-k kernel's skip-set bound and its 16 membership bits per posting, and the NumPy restatements
that prove from the inputs alone that a case is what it claims (test_jaccard_bound_cases_cpu.py).  A plain module like
jaccard_cases.py, on which it builds: no fixtures, no GPU.

The bound (csrc/ds_jaccard_impl.inc, "tighten / select"): under a cut, the skipped columns are the longest ascending-IDF
prefix of the query's columns whose mass stays below
    pre = coef * (max(sums_min, cut * maxint * (1 - 1e-5)) + maxint),   coef = cut / (1 + cut)
and whose columns all own a signature bit (`skipped_count`; band_edge=False is the bound without the max, the earlier one).

Every index here has three tiles of the geometry plus one row -- except the fixed 24,581-row case -- laid out in BANDS of
sums32 (ds_index_create orders the rows by sums32): the rows a case plants say where they lie, unique filler columns make
up the tiles.  The caller's row order is a random permutation of that order.
"""
import numpy as np

import jaccard_cases as jc

FILLER_IDF = 0.05
DECISIVE_K = (1, 10, 100)


# ---- restatements ------------------------------------------------------------------------------------------------------
def signature_bits(case):
    """{column: signature bit} as ds_index_create assigns them: the (up to) 128 longest lists in descending length, ties by
    ascending column, as long as a list holds at least 1 / 256 of the rows."""
    lengths = np.diff(case["rowptr"])
    n_rows = case["sums32"].shape[0]
    order = np.lexsort((np.arange(lengths.shape[0]), -lengths))[:128]
    bits = {}
    for bit, column in enumerate(order.tolist()):
        if lengths[column] * 256 < n_rows:
            break
        bits[column] = bit
    return bits


def prefix_masses(case, q):
    """The query's columns in ascending IDF order and the float64 mass of every prefix."""
    columns = jc.query_columns(case, q)
    idf = case["idf32"][columns].astype(np.float64)
    order = np.argsort(idf, kind="stable")
    return columns[order], np.cumsum(idf[order])


def pre_bound(case, q, cut, band_edge=True):
    maxint = float(np.float32(case["q_maxint"][q]))
    floor = float(case["sums32"].min())
    if band_edge:
        floor = max(floor, cut * maxint * (1.0 - 1e-5))
    return cut / (1.0 + cut) * (floor + maxint)


def skipped_count(case, q, cut, band_edge=True, bits=None):
    bits = signature_bits(case) if bits is None else bits
    columns, masses = prefix_masses(case, q)
    pre = pre_bound(case, q, cut, band_edge)
    count = 0
    while count < columns.shape[0] and masses[count] < pre and int(columns[count]) in bits:
        count += 1
    return count


def kth_value(case, q, k):
    """The k-th largest jaccard of query q and the next one below it (float64, every row)."""
    _, values = jc.jaccard_rows(case, q)
    ordered = np.sort(values[np.isfinite(values)])[::-1]
    return float(ordered[k - 1]), float(ordered[k])


def first_cut_floor(case, q, geometry, rows):
    """The smallest lower estimate the threshold bootstrap can give a row of `rows` (all in one tile): its score over the
    tile's LARGEST sums32 in place of its own (kernel: "No row's sums32 is read")."""
    scores, _ = jc.jaccard_rows(case, q)
    tile_min, tile_max = jc.tile_ranges(case, geometry)
    tile = jc.start_tile(case, q, (tile_min, tile_max))
    s = scores[rows].astype(np.float64)
    return float(np.min(s / (float(tile_max[tile]) + (float(case["q_maxint"][q]) - s))))


# ---- construction ------------------------------------------------------------------------------------------------------
def _spread(rng, lo, hi, n):
    """n distinct values strictly inside (lo, hi), in random order."""
    return lo + (hi - lo) * (rng.permutation(n) + 0.5) / max(n, 1)


def _assemble(geometry, rng, named_idf, groups, bands, queries, k, fillers=True, sizes=None, **meta):
    """groups: {name: (columns, sums32 targets)}; bands: per tile the [lo, hi) of sums32 that fillers make up to the tile's
    size (`sizes`, default three tiles and one row), the fillers below a third entry where a band has one.  Every row owns
    a filler column (IDF 0.05) unless fillers=False."""
    tile_rows = jc.GEOMETRY[geometry]["tile_rows"]
    sizes = [tile_rows] * (len(bands) - 1) + [1] if sizes is None else sizes
    named_idf = np.asarray(named_idf, dtype=np.float32)
    columns_of, targets, names = [], [], {}
    for name, (columns, sums) in groups.items():
        sums = np.asarray(sums, dtype=np.float64)
        names[name] = np.arange(len(targets), len(targets) + sums.shape[0])
        columns_of.extend([tuple(columns)] * sums.shape[0])
        targets.extend(sums.tolist())
    planted = np.asarray(targets)
    for band, size in zip(bands, sizes):
        lo, hi = band[:2]
        missing = size - int(np.sum((planted >= lo) & (planted < hi)))
        assert missing >= 0, ("a band holds more planted rows than its tile", lo, hi, missing)
        assert fillers or missing == 0
        columns_of.extend([()] * missing)
        targets.extend(_spread(rng, lo, band[2] if len(band) > 2 else hi, missing).tolist())
    targets = np.asarray(targets)
    n_rows, n_named = targets.shape[0], named_idf.shape[0]
    assert n_rows == sum(sizes)
    permutation = rng.permutation(n_rows)                      # caller's row of every row built here
    lengths = np.array([len(c) for c in columns_of])
    rows = np.repeat(permutation, lengths)
    cols = np.array([c for columns in columns_of for c in columns], dtype=np.int64)
    totals = np.zeros(n_rows)
    np.add.at(totals, rows, named_idf[cols].astype(np.float64))
    idf32 = named_idf
    if fillers:
        rows = np.concatenate((rows, permutation))
        cols = np.concatenate((cols, n_named + np.arange(n_rows)))
        idf32 = np.concatenate((named_idf, np.full(n_rows, FILLER_IDF, dtype=np.float32)))
        totals += float(np.float32(FILLER_IDF))
    extra = np.zeros(n_rows)
    extra[permutation] = targets
    extra -= totals
    assert extra.min() >= 0.0, "a planted row's sums32 lies below the total of its columns"
    index = jc.index_from_pairs(n_rows, idf32.shape[0], cols, rows, idf32=idf32, extra_sums=extra)
    case = jc._case(index, jc.queries_of(queries, index[2], index[3]), k, tiles=len(bands), **meta)
    case.update({name: np.sort(permutation[ids]) for name, ids in names.items()})
    return case


# ---- 1. the decisive column --------------------------------------------------------------------------------------------
def decisive_problem(geometry):
    """One query of five columns, in units of maxint = 10: S1 0.8, S2 1.2, D 2.2, E1 2.6, E2 3.2 (prefix masses 0.8, 2.0, 4.2,
    6.8, 10).  Under every cut the kernel can hold for it (0.499 .. 0.538) the bound without the band edge lies below 4.2 and
    the bound with it above: D is the one column more that is skipped, with more than 5 % of maxint to either side.
        full    560 rows with all five columns, sums32 18.87 .. 20.0, the top of the START tile (tile 2): jaccard 0.50 .. 0.53.
                They are the only rows of that tile with a positive score, so every threshold comes from them
        (a)     400 rows {S1, S2, D} -- skipped columns only -- with sums32 barely above their total: jaccard 0.42, the
                largest a row of skipped columns can reach (s <= mass < pre <= cut * maxint: "1e-4 below the cut" does not exist)
        (b)     150 rows {D, E2}, sums32 5.46 .. 6.06 (across the edge of tiles 0 and 1): jaccard 0.537 .. 0.508, the best rows
                of the index; their score is completed from the signature with the newly skipped D
        (c)     300 rows {S1, S2, E1}, sums32 5.10 .. 5.25, just below cut * maxint, in tile 0, which the sweep visits
    k = 1, 10, 100 (DECISIVE_K); tile 3 is one row out of every band's reach."""
    rng = np.random.RandomState(611)
    idf = [0.8, 1.2, 2.2, 2.6, 3.2]
    groups = {"full": (range(5), np.linspace(18.87, 20.0, 560)),
              "only_skipped": ((0, 1, 2), 4.26 + 0.0003 * np.arange(400)),
              "completed": ((2, 4), 5.46 + 0.004 * np.arange(150)),
              "below_band": ((0, 1, 3), 5.10 + 0.0005 * np.arange(300))}
    # (the fillers of tile 2 stay below the full rows, which are the tile's largest sums32)
    bands = [(0.2, 5.7), (5.7, 9.95), (10.0, 20.001, 18.8), (25.0, 26.0)]
    return _assemble(geometry, rng, idf, groups, bands, [list(range(5))], 10, decisive_column=2)


# ---- 2. membership bits 8..15 ------------------------------------------------------------------------------------------
def high_bits_problem(geometry):
    """Sixteen dense columns G0..G15 (IDF 0.25 + 0.001 g, lengths descending with g: G_g owns signature bit g), E1 2.9, E2 3.0;
    maxint 10.02; one query of all eighteen, k = 10.  Every cut (>= 0.448) skips exactly G0..G15 (mass 4.12).
        full     560 rows with all columns at the top of the start tile (jaccard 0.449 .. 0.455): the first threshold
        high     150 rows {G8..G15, E2}   jaccard 0.503 downwards, sums32 5.2 + 0.02 i
        low      150 rows {G0..G7, E2}    jaccard 0.499 downwards, sums32 5.08 + 0.005 i
        without  150 rows {E2}            jaccard below 0.25, with the sums32 of `high` + 0.001
        ballast  600 - 10 g rows {G_g} in the start tile (they order the lists' lengths)
    `high` and `without` differ only in the columns of bits 8..15, which the sweep has from the posting alone; the top ten
    are `high` and `low` rows, `without` lies below every cut."""
    rng = np.random.RandomState(815)
    idf = [0.25 + 0.001 * g for g in range(16)] + [2.9, 3.0]
    steps = 0.005 * np.arange(150)
    groups = {"full": (range(18), np.linspace(22.0, 22.3, 560)),
              "high": (tuple(range(8, 16)) + (17,), 5.2 + 4 * steps),
              "low": (tuple(range(8)) + (17,), 5.08 + steps),
              "without": ((17,), 5.201 + 4 * steps)}
    for g in range(16):
        groups["ballast%d" % g] = ((g,), _spread(rng, 10.1, 21.9, 600 - 10 * g))
    bands = [(0.2, 5.6), (5.6, 9.9), (10.05, 22.301, 21.95), (30.0, 31.0)]
    return _assemble(geometry, rng, idf, groups, bands, [list(range(18))], 10)


# ---- 3. round 4's trap -------------------------------------------------------------------------------------------------
CAPPED_UNITS = 32000            # an entry capped at (about) half of the fixed-point range: round 4's first tables
FIXED_ONE = 65000.0             # kFixedOne: the fixed-point value of the query's total mass


def capped_table_problem():
    """The same 24,581 rows in both geometries (narrow: two tiles and five rows; wide: one tile), three columns and nothing
    else: A 3.0, B 3.2, C 3.8, maxint 10, k = 1.  In the narrow geometry:
        tile 0   12,288 rows {A}, {B}, {C}, {A, C} with sums32 below 7.0
        tile 1   the START tile (sums32 7.05 .. 10.5): 300 rows {B, C} with sums32 7.05 .. 8.5 (jaccard 0.70 .. 0.61), the rest
                 {A}, {B}, {C} and {A, B} rows whose jaccard stays below 0.50.  k = 1: the first cut is the best sample, 7 /
                 (10.5 + 3) = 0.52, which only the 300 pass -- at least max(k, 16) and fewer than the buffer holds, so the
                 tile ends in a selection and the cut becomes their best, 0.70: cut * maxint = 7.0 > 6.2, A AND B are skipped,
                 62 % of the query's mass
        tile 2   five rows ABOVE the start tile, swept sparsely over C alone: the winner {A, B, C} with sums32 13 (jaccard
                 0.77) and four {A} rows above it.  The winner is reached through its C posting only: its essential score is
                 3.8 against the tile's gate coef * (13 + 10) = 9.4, so it passes only if the membership bits credit it with
                 the whole 6.2 of A and B.  A table entry capped at 32,000 of the 65,000 fixed-point units (4.9) loses it.
    In the wide geometry all rows are one densely scanned tile (the same answer, no sweep)."""
    rng = np.random.RandomState(424)
    groups = {"a0": ((0,), _spread(rng, 3.06, 7.0, 5000)), "b0": ((1,), _spread(rng, 3.3, 7.0, 4000)),
              "c0": ((2,), _spread(rng, 3.9, 7.0, 2288)), "ac0": ((0, 2), _spread(rng, 6.85, 7.0, 1000)),
              "bc": ((1, 2), np.linspace(7.05, 8.5, 300)),
              "a1": ((0,), _spread(rng, 7.1, 10.5, 4000)), "b1": ((1,), _spread(rng, 7.1, 10.5, 4000)),
              "ab1": ((0, 1), _spread(rng, 8.6, 10.5, 2988)), "c1": ((2,), _spread(rng, 7.1, 10.5, 1000)),
              "winner": ((0, 1, 2), [13.0]), "above": ((0,), [13.5, 14.0, 14.5, 15.0])}
    return _assemble("narrow", rng, [3.0, 3.2, 3.8], groups, [(0.0, 7.04), (7.04, 12.0), (12.0, 16.0)], [[0, 1, 2]], 1,
                     fillers=False, sizes=[12288, 12288, 5])


# ---- 4. padding, 5. no threshold ---------------------------------------------------------------------------------------
PADDING_LISTS = (1, 2, 3, 5)


def padding_problem(geometry):
    """S (IDF 3, held by half of all other rows) and four rare columns P1, P2, P3, P5 (IDF 7) that hold 1, 2, 3 and 5 rows in
    EACH of the three full tiles -- lists of one or two quads per tile, padded -- and P1 also the single row of the last,
    partial tile.  Query n = {S, Pn} at k = the rows of Pn (4, 6, 9, 15): the answer is exactly the rows next to the
    padding (jaccard >= 0.45; a row with S alone stays below 0.22).  Queries 4 and 5 are {P2} and {P3} alone, for k = 10:
    six and nine positive rows, no threshold ever (cut 0), the literal kernel answers ("few")."""
    rng = np.random.RandomState(97)
    bands = [(7.1, 8.5), (8.5, 9.95), (10.0, 12.0), (12.4, 12.6)]
    groups = {}
    for column, n in enumerate(PADDING_LISTS, start=1):
        sums = np.concatenate([_spread(rng, lo + 0.01, hi - 0.01, n) for lo, hi in bands[:3]] + ([[12.5]] if n == 1 else []))
        groups["p%d" % n] = ((column,), sums)
    tile_rows = jc.GEOMETRY[geometry]["tile_rows"]
    for tile, (lo, hi) in enumerate(bands[:3]):
        groups["s%d" % tile] = ((0,), _spread(rng, lo + 0.001, hi - 0.001, tile_rows // 2))
    lists = [[0, column] for column in range(1, 5)] + [[2], [3]]
    case = _assemble(geometry, rng, [3.0, 7.0, 7.0, 7.0, 7.0], groups, bands, lists, None)
    case["k_of_query"] = [int(case["p%d" % n].shape[0]) for n in PADDING_LISTS] + [10, 10]
    return case
