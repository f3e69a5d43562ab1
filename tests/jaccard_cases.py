"""Inputs for the Jaccard top-k kernel built to reach ONE named path each, in either of its two geometries, and the NumPy
restatements that prove from the inputs alone that a case is what it claims (test_jaccard_cases_cpu.py).  A plain module
like duplicates_cases.py: no fixtures, no GPU.  The generators are vectorised (no Python loop over rows).

GEOMETRY mirrors the #defines of csrc/ds_jaccard_narrow.hip / ds_jaccard_wide.hip and the tile sizes of ds_common.h; the
CPU test compares the two, so a retune has to move this table -- and with it what the GPU tests cover -- on purpose.

A case is a dict: the eight arrays of a ds_jaccard_topk call (`arrays(case)`) plus what the case knows about itself
(tile counts, the rows it planted, the tile that overflows ...).
"""
import numpy as np

GEOMETRY = {"narrow": dict(tile_rows=12288, threads=256, candidates=768, ptr_tiles=1, epoch_tiles=4),
            "wide": dict(tile_rows=28672, threads=512, candidates=1472, ptr_tiles=3, epoch_tiles=16)}
GEOMETRIES = tuple(GEOMETRY)
SELECT_SLACK = 128          # kSelectSlack
SPARSE_QUADS = 4096         # JaccardArgs::sparse_quads: a selection whose essential columns average more quads per tile scans densely
MAX_QUERY_COLUMNS = 128     # kMaxQueryColumns
MAX_SELECT_K = 512          # kMaxSelectK


def probe_max_k(geometry):
    """kProbeMaxK: the largest k whose first threshold comes from ONE sample per thread."""
    return GEOMETRY[geometry]["threads"] // 4


def k_classes(geometry):
    """How the first threshold of a query is found, by k (inclusive ranges): launch() and the bootstrap at the dense scan."""
    p = probe_max_k(geometry)
    return {"first_sample": (1, p), "second_sample": (p + 1, 2 * p), "flood": (2 * p + 1, MAX_SELECT_K)}


def k_class_edges(geometry):
    """Both sides of every class edge, and the largest k the selection kernels take."""
    p = probe_max_k(geometry)
    return (p, p + 1, 2 * p, 2 * p + 1, MAX_SELECT_K)


def select_trigger(geometry):
    """kSelectTrigger: a selection leaves at most this many candidates in the buffer."""
    return GEOMETRY[geometry]["candidates"] - SELECT_SLACK


def pointer_span(geometry, n_columns_of_query, n_tiles):
    """`span` of the fast kernel: the tiles whose list pointers the LDS cache holds for a query of n columns."""
    g = GEOMETRY[geometry]
    return min(n_tiles, max(g["ptr_tiles"], MAX_QUERY_COLUMNS * (g["ptr_tiles"] + 1) // n_columns_of_query - 1))


def arrays(case):
    return tuple(case[name] for name in ("rowptr", "truth_idx", "idf32", "sums32", "q_rowptr", "q_cols", "q_maxint", "k"))


# ---- index and query construction -------------------------------------------------------------------------------------
def row_sums32(n_rows, cols, rows, idf32):
    """sums32 as match_maker.py:174 computes it: per row the sequential float32 sum of its columns' idf values in
    ascending column order.  (cols, rows) sorted by (column, row)."""
    by_row = np.argsort(rows, kind="stable")                     # ascending column inside a row
    counts = np.bincount(rows, minlength=n_rows)
    starts = np.concatenate(([0], np.cumsum(counts)))[:-1]
    values = idf32[cols[by_row]]
    out = np.zeros(n_rows, dtype=np.float32)
    for position in range(int(counts.max()) if counts.shape[0] else 0):      # a loop over the LONGEST row's columns
        active = np.nonzero(counts > position)[0]
        out[active] = out[active] + values[starts[active] + position]
    return out


def index_from_pairs(n_rows, n_columns, cols, rows, idf32=None, extra_sums=None):
    """CSR inverted index from (column, row) pairs (duplicates dropped); idf = ln(N / df) as match_maker.py:135-142 unless
    `idf32` is given (the C ABI takes any); sums32 = row_sums32 (+ extra_sums[row]: the C ABI allows more).
    Returns rowptr, truth_idx, idf32, idf64, sums32."""
    keys = np.unique(np.asarray(cols, dtype=np.int64) * n_rows + np.asarray(rows, dtype=np.int64))
    cols, rows = keys // n_rows, keys % n_rows
    lengths = np.bincount(cols, minlength=n_columns)
    rowptr = np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
    if idf32 is None:
        idf64 = np.log(n_rows / np.maximum(lengths, 1))
        idf32 = idf64.astype(np.float32)
    else:
        idf32 = np.asarray(idf32, dtype=np.float32)
        idf64 = idf32.astype(np.float64)
    sums32 = row_sums32(n_rows, cols, rows, idf32)
    if extra_sums is not None:
        sums32 = (sums32 + extra_sums.astype(np.float32)).astype(np.float32)
    return rowptr, rows.astype(np.int32), idf32, idf64, sums32


def build_index(n_rows, columns, extra_sums=None):
    """The same from {column id: sorted row array}."""
    ids = sorted(columns)
    cols = np.concatenate([np.full(len(columns[c]), c, dtype=np.int64) for c in ids])
    rows = np.concatenate([np.asarray(columns[c], dtype=np.int64) for c in ids])
    return index_from_pairs(n_rows, max(ids) + 1, cols, rows, extra_sums=extra_sums)


def queries_of(column_lists, idf32, idf64):
    """Queries as match_maker.py:196-197 makes them: ascending columns of non-zero idf, max_intersection_possible = their
    float64 idf total."""
    kept = [np.array(sorted(c for c in columns if idf32[c] != 0), dtype=np.int32) for columns in column_lists]
    q_rowptr = np.concatenate(([0], np.cumsum([len(c) for c in kept]))).astype(np.int64)
    q_cols = np.concatenate(kept).astype(np.int32)
    q_maxint = np.array([float(sum(float(idf64[c]) for c in columns)) for columns in kept])
    return q_rowptr, q_cols, q_maxint


def _case(index, queries, k, **meta):
    rowptr, truth_idx, idf32, _, sums32 = index
    q_rowptr, q_cols, q_maxint = queries
    return dict(rowptr=rowptr, truth_idx=truth_idx, idf32=idf32, sums32=sums32, q_rowptr=q_rowptr, q_cols=q_cols,
                q_maxint=q_maxint, k=k, **meta)


# ---- restatements ------------------------------------------------------------------------------------------------------
def tiles_of(case, geometry):
    n_rows, tile_rows = case["sums32"].shape[0], GEOMETRY[geometry]["tile_rows"]
    return (n_rows + tile_rows - 1) // tile_rows


def internal_order(case):
    """ds_index_create's row order unless DS_SORT_ROWS=0: ascending sums32, ties by ascending row.  position -> row."""
    return np.argsort(case["sums32"], kind="stable")


def query_columns(case, q):
    return case["q_cols"][case["q_rowptr"][q]:case["q_rowptr"][q + 1]]


def jaccard_rows(case, q):
    """fast_jaccard of query q over every row (match_maker.py:16-50): float32 scores summed in the query's column order,
    float64(s) / (float64(sums) + (maxint - float64(s))).  Returns (scores float32[N], jaccard float64[N])."""
    scores = np.zeros(case["sums32"].shape[0], dtype=np.float32)
    for column in query_columns(case, q):
        members = case["truth_idx"][case["rowptr"][column]:case["rowptr"][column + 1]]
        scores[members] = scores[members] + case["idf32"][column]
    s = scores.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return scores, s / (case["sums32"].astype(np.float64) + (float(case["q_maxint"][q]) - s))


def columns_of_rows(case, wanted):
    """{row: tuple of its columns, ascending} for the rows in `wanted`."""
    columns = np.repeat(np.arange(case["rowptr"].shape[0] - 1), np.diff(case["rowptr"]))
    pick = np.nonzero(np.isin(case["truth_idx"], wanted))[0]
    order = np.lexsort((columns[pick], case["truth_idx"][pick]))
    rows, cols = case["truth_idx"][pick][order], columns[pick][order]
    cuts = np.nonzero(np.diff(rows))[0] + 1
    return {int(r[0]): tuple(c.tolist()) for r, c in zip(np.split(rows, cuts), np.split(cols, cuts))} if rows.shape[0] else {}


def quads_upper_bound(case, q, geometry):
    """No fewer posting quads than the index stores for ALL of query q's columns: per (column, tile) the even and the odd
    rows are padded to whole quads each, i.e. at most postings / 4 + 2 quads."""
    lengths = np.diff(case["rowptr"])[query_columns(case, q)]
    return int(np.sum(lengths // 4 + 1)) + 2 * lengths.shape[0] * tiles_of(case, geometry)


def jaccard_of(case, q, wanted):
    """jaccard_rows for the rows `wanted` only (membership by binary search in every column's list)."""
    wanted = np.asarray(wanted, dtype=np.int64)
    scores = np.zeros(wanted.shape[0], dtype=np.float32)
    for column in query_columns(case, q):
        members = case["truth_idx"][case["rowptr"][column]:case["rowptr"][column + 1]]
        if members.shape[0] == 0:
            continue
        at = np.minimum(np.searchsorted(members, wanted), members.shape[0] - 1)
        hit = members[at] == wanted
        scores[hit] = scores[hit] + case["idf32"][column]
    s = scores.astype(np.float64)
    return s / (case["sums32"][wanted].astype(np.float64) + (float(case["q_maxint"][q]) - s))


def tile_ranges(case, geometry):
    """(tile_sums_min, tile_sums_max) of the index with its rows in sums32 order."""
    tile_rows = GEOMETRY[geometry]["tile_rows"]
    ordered = np.sort(case["sums32"], kind="stable")
    firsts = np.arange(0, ordered.shape[0], tile_rows)
    return ordered[firsts], ordered[np.minimum(firsts + tile_rows, ordered.shape[0]) - 1]


def start_tile(case, q, ranges):
    """Where the sweep of query q starts: the tiles whose largest sums32 lies below float32(max_intersection_possible)."""
    return min(int(np.sum(ranges[1] < np.float32(case["q_maxint"][q]))), ranges[1].shape[0] - 1)


def band_tiles(case, q, ranges, expected_rows):
    """Tiles the sweep of query q cannot leave out, with the rows in sums32 order.  The kernel leaves a side of its start
    tile once `tile_sums_min * cut > maxint * 1.00001` (above) or `tile_sums_max < cut * maxint * 0.99999` (below); its cut
    never exceeds the k-th largest jaccard -- below the smallest value among the reference's answer plus 2e-6 (the
    reference's 1e-6 and the float32 rounding of its heap minimum), which is used here -- so the band under THAT value is a subset of every band the kernel works with."""
    tile_min, tile_max = ranges
    maxint = float(case["q_maxint"][q])
    start = start_tile(case, q, ranges)
    cut = max(float(np.min(jaccard_of(case, q, expected_rows))) + 2e-6, 0.0)
    in_band = (tile_min.astype(np.float64) * cut <= maxint) & (tile_max.astype(np.float64) >= cut * maxint)
    last = start
    while last + 1 < tile_min.shape[0] and in_band[last + 1]:
        last += 1
    first = start
    while first - 1 >= 0 and in_band[first - 1]:
        first -= 1
    return last - first + 1


def multi_epoch_queries(case, geometry, expected):
    """The queries whose sweep must visit MORE sparse tiles than one epoch holds, whatever the order of events in the kernel:
    the band of band_tiles has more than epoch_tiles tiles besides the start tile (the only one scanned densely once the
    bootstrap of k <= 2 * probe_max_k has set a threshold there), and the posting quads of ALL the query's columns average
    at most sparse_quads per tile (the essential columns are a subset, so every selection chooses the sparse mode)."""
    ranges = tile_ranges(case, geometry)
    epoch, n_tiles = GEOMETRY[geometry]["epoch_tiles"], tiles_of(case, geometry)
    assert case["k"] <= 2 * probe_max_k(geometry)
    return np.array([band_tiles(case, q, ranges, expected[q]) - 1 > epoch and
                     quads_upper_bound(case, q, geometry) <= SPARSE_QUADS * n_tiles
                     for q in range(case["q_maxint"].shape[0])])


# ---- random indexes (test_gpu_jaccard.py's _random_problem / _tie_problem, vectorised) -------------------------------------
def random_problem(rng, n_truth, n_columns, n_queries, mean_cols=12, heavy=6, duplicates=0, k=10):
    """Random inverted index with a few heavy columns; queries reuse most of a truth row's columns and add a few.
    duplicates = d: rows 1..d-1 are twins of row 0 (same columns, same sums32)."""
    per_row = np.clip(rng.poisson(mean_cols, n_truth), 1, 60)
    rows = np.repeat(np.arange(n_truth, dtype=np.int64), per_row)
    cols = rng.randint(heavy, n_columns, rows.shape[0]).astype(np.int64)
    heavy_rows, heavy_cols = np.nonzero(rng.rand(n_truth, heavy) < 0.3)
    rows, cols = np.concatenate((rows, heavy_rows)), np.concatenate((cols, heavy_cols))
    if duplicates:
        twin = rows < duplicates
        first = np.unique(cols[rows == 0])
        rows = np.concatenate((rows[~twin], np.repeat(np.arange(duplicates, dtype=np.int64), first.shape[0])))
        cols = np.concatenate((cols[~twin], np.tile(first, duplicates)))
    index = index_from_pairs(n_truth, n_columns, cols, rows)
    rowptr, truth_idx, idf32, idf64, _ = index
    column_of = np.repeat(np.arange(n_columns), np.diff(rowptr))
    lists = []
    for q in range(n_queries):
        base = column_of[truth_idx == rng.randint(n_truth)] if rng.rand() < 0.7 else np.zeros(0, dtype=np.int64)
        extra = rng.randint(0, n_columns, rng.randint(1, 10))
        lists.append(np.unique(np.concatenate((base[rng.rand(base.shape[0]) < 0.8], extra))).tolist())
    if duplicates:                      # every fourth query IS the duplicated row: the ties sit at the top
        for q in range(0, n_queries, 4):
            lists[q] = column_of[truth_idx == 0].tolist()
    return _case(index, queries_of(lists, idf32, idf64), k, duplicates=duplicates)


def tie_problem(geometry, duplicates=6000):
    """3 tiles of the geometry, 6,000 twin rows, 40 queries of which ten equal the twins."""
    return random_problem(np.random.RandomState(5), 3 * GEOMETRY[geometry]["tile_rows"], 2000, 40, duplicates=duplicates)


def ragged_problem(geometry):
    """3 tiles plus ONE row (a last tile of a single row), 96 queries."""
    return random_problem(np.random.RandomState(99), 3 * GEOMETRY[geometry]["tile_rows"] + 1, 3000, 96)


# ---- the sweeps ----------------------------------------------------------------------------------------------------------
def second_posting_problem(geometry="narrow"):
    """48 queries over 4 tiles.  Twelve rare columns co-occur heavily (every "cluster" row holds three or four of them), six
    dense columns are what a threshold lets the kernel skip, every row carries three filler columns (no two rows are
    twins).  Most candidate rows so receive postings from two or three essential columns inside one sparse tile: the
    collect sweep meets a row's SECOND posting after another lane took its score.  The row counts scale with the tile; a
    dense column holds 0.4 of the narrow rows and 0.17 of the wide ones, i.e. 1,229 quads per tile in both: with three of the
    six skipped the essential quads are below sparse_quads and the tiles are swept sparsely."""
    rng = np.random.RandomState(31)
    tile_rows = GEOMETRY[geometry]["tile_rows"]
    n_rows, scale = 4 * tile_rows, tile_rows / 12288.0
    cols, rows = [], []
    for dense in range(6):                                       # signature-bearing, skipped after the first threshold
        members = rng.choice(n_rows, int(0.4 / scale * n_rows), replace=False)      # the same quads per tile in both geometries
        cols.append(np.full(members.shape[0], dense))
        rows.append(members)
    n_cluster, n_fillers = int(2400 * scale), int(3000 * scale)
    cluster_rows = rng.choice(n_rows, n_cluster, replace=False)          # spread over all four tiles
    picked = 6 + np.argsort(rng.rand(n_cluster, 12), axis=1)[:, :4]      # four different rare columns, the last one optional
    keep = np.arange(4)[None, :] < rng.randint(3, 5, n_cluster)[:, None]
    cols.append(picked[keep])
    rows.append(np.repeat(cluster_rows, 4).reshape(-1, 4)[keep])
    for rare in range(6, 18):                                            # rows that hold only this rare column
        cols.append(np.full(int(150 * scale), rare))
        rows.append(rng.choice(n_rows, int(150 * scale), replace=False))
    cols.append((18 + rng.randint(0, n_fillers, (n_rows, 3))).ravel())
    rows.append(np.repeat(np.arange(n_rows), 3))
    index = index_from_pairs(n_rows, 18 + n_fillers, np.concatenate(cols), np.concatenate(rows))
    lists = [list(range(6)) + (6 + rng.choice(12, 4, replace=False)).tolist() for _ in range(48)]
    return _case(index, queries_of(lists, index[2], index[3]), 10, tiles=4, cluster_rows=np.sort(cluster_rows))


def descending_epochs_tiles(geometry):
    """Two full epochs plus three tiles in the wide geometry; the narrow case keeps its 13 tiles (three epochs plus one)."""
    return 13 if geometry == "narrow" else 2 * GEOMETRY[geometry]["epoch_tiles"] + 3


# columns per query of the three families (inclusive), and the longest row a family-three query is grown from
_FAMILIES = {"narrow": dict(one=(64, 128), two=(30, 50), short_row=16, extra=6, per_row=(3, 100)),
             "wide": dict(one=(64, 128), two=(20, 30), short_row=4, extra=2, per_row=(3, 20))}


def descending_epochs_problem(geometry="narrow"):
    """13 narrow / 35 wide tiles, rows of 3..100 (wide: 3..20, to keep generation and oracle short) columns: in the internal
    sums32 order the long rows are the last tiles.  Three families of 24 queries, top-100 (a weak cut: the sweeps run far):
    one   64..128 random columns -- they start in the LAST tiles and descend towards tile 0 with a pointer block
          (narrow span 1..3, wide 3..7) SHORTER than an epoch (4 / 16 tiles);
    two   30..50 (wide 20..30) random columns: a span (4..7 / 16..24) of an epoch or more, below family three's;
    three the columns of a short row plus six (wide: two) random ones -- they start within an epoch of tile 0 with a span
          (10..13 / 35, the whole index) LONGER than the tiles below the start.
    Families one and three are the two corners of `block_start = max(0, min(b, epoch_last - span + 1))`."""
    rng = np.random.RandomState(1747)
    family = _FAMILIES[geometry]
    n_tiles = descending_epochs_tiles(geometry)
    n_rows, n_columns = n_tiles * GEOMETRY[geometry]["tile_rows"], 3000
    per_row = rng.randint(family["per_row"][0], family["per_row"][1] + 1, n_rows)
    rows = np.repeat(np.arange(n_rows, dtype=np.int64), per_row)
    # column popularity: a few dense columns (signature bits, skipped under a threshold), a long flat tail
    weights = 1.0 / (np.arange(n_columns) + 20.0)
    cols = rng.choice(n_columns, rows.shape[0], p=weights / weights.sum())
    index = index_from_pairs(n_rows, n_columns, cols, rows)
    rowptr, truth_idx, idf32, idf64, _ = index
    counts = np.bincount(truth_idx, minlength=n_rows)
    short_rows = np.nonzero(counts <= family["short_row"])[0]
    column_of = np.repeat(np.arange(n_columns), np.diff(rowptr))
    lists = []
    for name in ("one", "two"):
        for _ in range(24):
            lists.append(rng.choice(n_columns, rng.randint(family[name][0], family[name][1] + 1), replace=False).tolist())
    seeds = short_rows[rng.randint(short_rows.shape[0], size=24)]
    own = columns_of_rows(dict(rowptr=rowptr, truth_idx=truth_idx), seeds)
    for row in seeds:
        lists.append(sorted(set(own[int(row)]) | set(rng.choice(n_columns, family["extra"], replace=False).tolist())))
    return _case(index, queries_of(lists, idf32, idf64), 100, tiles=n_tiles,
                 families=dict(one=range(0, 24), two=range(24, 48), three=range(48, 72)))


def redo_problem(geometry="narrow", tied=False):
    """epoch_tiles + 2 tiles (6 / 18), k = 100, rows kept in the caller's order (DS_SORT_ROWS=0).  Tile 0 holds 300 rows with
    column C (they set the first threshold); tile 2 -- the SECOND tile of the epoch of sparse tiles 1..epoch_tiles -- holds
    candidates + 230 rows (998 / 1,702) with column A whose jaccard beats every C row: more than the candidate buffer takes.
    tied = False: their values are all different, a tighter threshold prunes them and the repeated epoch fits.  tied =
    True: they are equal (same sums32, a different filler column each, so no twins): no threshold separates them and the
    fast kernel must give up.  Almost no postings: every tile after the first is sparse."""
    rng = np.random.RandomState(47)
    g = GEOMETRY[geometry]
    tile_rows, n_strong = g["tile_rows"], g["candidates"] + 230
    n_rows = (g["epoch_tiles"] + 2) * tile_rows
    a_rows = np.sort(2 * tile_rows + rng.choice(tile_rows, n_strong, replace=False))
    c_rows = np.sort(rng.choice(tile_rows, 300, replace=False))
    cols = np.concatenate((np.zeros(n_strong, np.int64), np.ones(300, np.int64), 2 + np.arange(n_strong)))
    rows = np.concatenate((a_rows, c_rows, a_rows))                     # a filler column of its own: no twins
    extra = np.zeros(n_rows, dtype=np.float64)
    extra[c_rows] = 60.0 + 0.01 * np.arange(300)                        # weak rows: jaccard ~ 0.09
    if not tied:
        extra[a_rows] = 0.005 * np.arange(n_strong)                     # strong rows, all different
    index = index_from_pairs(n_rows, 2 + n_strong, cols, rows, extra_sums=extra)
    return _case(index, queries_of([[0, 1]], index[2], index[3]), 100, tiles=g["epoch_tiles"] + 2, strong_rows=a_rows,
                 weak_rows=c_rows, overflowing_tile=2, tied=tied)


# ---- the hand-over ledger ------------------------------------------------------------------------------------------------
FEW_K = (1, 10, 100)


def few_problem(geometry):
    """Reason 5, `m < k` after the last tile: nine columns held by exactly k-1, k and k+1 rows for k in {1, 10, 100} (0, 1, 2,
    9, 10, 11, 99, 100, 101 rows; column j of `few_sizes`), each the ONLY column of its query, so the rows with a positive
    score are exactly its holders.  Every row also has a column of its own (no twins) and a sums32 that places it in the internal
    sums32 order wherever the case wants it: a column's holders alternate between the first two tiles of the index: 2 tiles plus 5 rows.  case["queries_of_k"][k] are the
    three queries of k, in the order k-1, k, k+1 holders."""
    rng = np.random.RandomState(55)
    sizes = [k + d for k in FEW_K for d in (-1, 0, 1)]
    n_rows = 2 * GEOMETRY[geometry]["tile_rows"] + 5
    holders = rng.choice(n_rows, sum(sizes), replace=False)             # disjoint sets
    cols = np.concatenate((np.repeat(np.arange(len(sizes)), sizes), len(sizes) + np.arange(n_rows)))
    rows = np.concatenate((holders, np.arange(n_rows)))
    rowptr, truth_idx, idf32, idf64, _ = index_from_pairs(n_rows, len(sizes) + n_rows, cols, rows)
    # The holders of a column alternate between the first two tiles of the internal order: every row gets a position there
    # (the holders theirs, the others the rest at random) and sums32 = ln N (the own column) + 12 + 5 * position / N, which
    # ascends with the position whether or not the row holds a counted column (idf <= ln N < 12: never below the row's total)
    tile_rows = GEOMETRY[geometry]["tile_rows"]
    in_tile = np.concatenate([np.arange(size) % 2 for size in sizes])
    slots = np.empty(in_tile.shape[0], dtype=np.int64)
    for tile in (0, 1):
        slots[in_tile == tile] = tile * tile_rows + rng.choice(tile_rows, int(np.sum(in_tile == tile)), replace=False)
    position = np.empty(n_rows, dtype=np.int64)
    position[holders] = slots
    others = np.setdiff1d(np.arange(n_rows), holders)
    position[others] = rng.permutation(np.setdiff1d(np.arange(n_rows), slots))
    sums32 = (idf32[len(sizes):] + (12.0 + 5.0 * position / n_rows).astype(np.float32)).astype(np.float32)
    index = (rowptr, truth_idx, idf32, idf64, sums32)
    queries = queries_of([[j] for j in range(len(sizes))], idf32, idf64)
    return _case(index, queries, None, tiles=3, few_sizes=sizes,
                 queries_of_k={k: [3 * i, 3 * i + 1, 3 * i + 2] for i, k in enumerate(FEW_K)})


def select_queries(case, which, k):
    """The case restricted to the queries `which`, at k."""
    lists = [query_columns(case, q) for q in which]
    out = dict(case)
    out.update(q_rowptr=np.concatenate(([0], np.cumsum([len(c) for c in lists]))).astype(np.int64),
               q_cols=np.concatenate(lists).astype(np.int32), q_maxint=case["q_maxint"][list(which)].copy(), k=k)
    return out


SHAPE_MAXINT = ("total", "total * 0.9995", "total * 0.99", "0.0", "-1.0", "1e30", "inf", "nan")


def shape_problem(geometry):
    """Reason 0, the conditions on the query's shape at the head of the fast kernel:
        n > 128  or  not (maxint > 0)  or  not (maxint < 1e30)  or  float32(maxint) < mass * 0.999f
    where mass is the idf total of the query's columns, rounded up.  Eight queries with the SAME 12 columns differ only in
    max_intersection_possible (SHAPE_MAXINT), then one of 128 and one of 129 columns with their exact totals.
    case["handed_over"] names the queries the conditions send to the literal kernel.  2 tiles plus 77 rows, k = 10."""
    rng = np.random.RandomState(528)
    n_rows = 2 * GEOMETRY[geometry]["tile_rows"] + 77
    base = random_problem(rng, n_rows, 1500, 1)
    rowptr, truth_idx, idf32 = base["rowptr"], base["truth_idx"], base["idf32"]
    idf64 = np.log(n_rows / np.maximum(np.diff(rowptr), 1))
    column_of = np.repeat(np.arange(rowptr.shape[0] - 1), np.diff(rowptr))
    counts = np.bincount(truth_idx, minlength=n_rows)
    twelve = column_of[truth_idx == np.nonzero(counts == 12)[0][0]]      # the columns of a row that has twelve
    used = np.nonzero((np.diff(rowptr) > 0) & (idf32 != 0))[0]
    lists = [twelve.tolist()] * len(SHAPE_MAXINT) + [rng.choice(used, 128, replace=False).tolist(),
                                                      rng.choice(used, 129, replace=False).tolist()]
    q_rowptr, q_cols, q_maxint = queries_of(lists, idf32, idf64)
    total = q_maxint[0]
    q_maxint[:len(SHAPE_MAXINT)] = [total, total * 0.9995, total * 0.99, 0.0, -1.0, 1e30, np.inf, np.nan]
    base.update(q_rowptr=q_rowptr, q_cols=q_cols, q_maxint=q_maxint, k=10, tiles=3,
                handed_over=np.array([False, False, True, True, True, True, True, True, False, True]))
    return base


def overflow_dense_problem(geometry, tied):
    """Reason 3: more rows above the cut inside ONE densely scanned tile than the candidate buffer holds.  3 tiles, rows kept
    in the caller's order (DS_SORT_ROWS=0), k = 100, idf values chosen freely (the C ABI takes any non-negative ones):
        columns  A = 0 (idf 3), C = 1 (idf 3), D1 = 2 and D2 = 3 (idf 1.5 each, held by EVERY row), a filler (idf 0.5) per A row
        tile 0   300 weak rows {C, D1, D2}, sums32 116 + 0.01 i: jaccard ~ 0.050 -- they set the first cut
        tile 1   candidates + 230 strong rows {A, D1, D2, own filler} (998 / 1,702), jaccard 0.33..0.63, far above that cut
        the rest {D1, D2} with sums32 1000: jaccard 0.003, below every cut
    D1 and D2 keep the tiles dense: under the first cut neither can be skipped (idf 1.5 > coef * (min sums32 + maxint) ~
    0.74), and together they are 2 * tile_rows / 4 quads per tile, above sparse_quads = 4096 in both geometries.
    tied = False: the strong rows' sums32 all differ (steps of 0.005 in random order), the retry under the tightened cut
    fits.  tied = True: equal sums32, equal jaccard, no twins (own filler): no cut and no admission floor separates them."""
    rng = np.random.RandomState(1311)
    g = GEOMETRY[geometry]
    tile_rows, n_strong = g["tile_rows"], g["candidates"] + 230
    n_rows = 3 * tile_rows
    strong = np.sort(tile_rows + rng.choice(tile_rows, n_strong, replace=False))
    weak = np.sort(rng.choice(tile_rows, 300, replace=False))
    everyone = np.arange(n_rows)
    cols = np.concatenate((np.zeros(n_strong, np.int64), np.ones(300, np.int64), np.full(n_rows, 2), np.full(n_rows, 3),
                           4 + np.arange(n_strong)))
    rows = np.concatenate((strong, weak, everyone, everyone, strong))
    idf32 = np.concatenate(([3.0, 3.0, 1.5, 1.5], np.full(n_strong, 0.5))).astype(np.float32)
    extra = np.full(n_rows, 997.0)                                       # {D1, D2} = 3: sums32 1000
    extra[weak] = 110.0 + 0.01 * np.arange(300)                          # {C, D1, D2} = 6
    extra[strong] = 0.0 if tied else 0.005 * rng.permutation(n_strong)   # {A, D1, D2, filler} = 6.5
    index = index_from_pairs(n_rows, 4 + n_strong, cols, rows, idf32=idf32, extra_sums=extra)
    return _case(index, queries_of([[0, 1, 2, 3]], index[2], index[3]), 100, tiles=3, strong_rows=strong, weak_rows=weak,
                 overflowing_tile=1, tied=tied)
