"""Inputs and restatements for the tests of the device index build (test_index_build_cpu.py, test_gpu_index_build.py).

`duplicate_ranks_rule` restates the duplicate-rank rule of ds::duplicate_ranks in NumPy, with the truncated hashes of
ds_index_build_option("duplicate_hash_bits", b).  `internal_csr` restates the internal row order of ds_index_create
(stable, ascending in its own key of sums32), on which the ranks of an index are computed.  The hand-made CSR and the
twins problem are the inputs of the GPU tests.

`expected_image` restates the whole image of an index from the documented rule and `image_digest`
the words of ds_index_image_digest on it; `adversarial_problem` generates indexes from a seed and the named edge problems
(`named_problems`) put single stages of the device build at their edges (test_index_build_edges_cpu.py,
test_gpu_index_build_edges.py).  Nothing here calls the library."""
import functools

import numpy as np

NARROW, WIDE = 12288, 28672


def mix64(x):
    """splitmix64 finaliser on uint64 arrays (ds_common.h: mix64)."""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x ^ (x >> np.uint64(30))
        x = x * np.uint64(0xbf58476d1ce4e5b9)
        x = x ^ (x >> np.uint64(27))
        x = x * np.uint64(0x94d049bb133111eb)
        x = x ^ (x >> np.uint64(31))
    return x


def order_key(sums32):
    """ds_index_create's order key: the bits with all bits flipped for a set sign, else the sign bit flipped; -0.0 and
    NaN get no special case."""
    bits = np.ascontiguousarray(sums32, dtype=np.float32).view(np.uint32)
    return np.where(bits >> 31 != 0, ~bits, bits ^ np.uint32(0x80000000)).astype(np.uint32)


def csr_from_pairs(n_columns, cols, rows):
    """(rowptr int64[V + 1], truth_idx int32[nnz]) of distinct (column, row) pairs, lists ascending."""
    cols, rows = np.asarray(cols, dtype=np.int64), np.asarray(rows, dtype=np.int64)
    order = np.lexsort((rows, cols))
    cols, rows = cols[order], rows[order]
    rowptr = np.zeros(n_columns + 1, dtype=np.int64)
    np.cumsum(np.bincount(cols, minlength=n_columns), out=rowptr[1:])
    return rowptr, rows.astype(np.int32)


def pairs_of(rowptr, truth_idx):
    rowptr = np.asarray(rowptr, dtype=np.int64)
    return np.repeat(np.arange(rowptr.shape[0] - 1, dtype=np.int64), np.diff(rowptr)), np.asarray(truth_idx, dtype=np.int64)


def internal_csr(rowptr, truth_idx, sums32, sort_rows=True):
    """(rowptr, truth_idx in internal rows, sums32 in internal order, original row of every internal row)."""
    sums32 = np.ascontiguousarray(sums32, dtype=np.float32)
    n = sums32.shape[0]
    original = np.argsort(order_key(sums32), kind="stable") if sort_rows else np.arange(n)
    position = np.empty(n, dtype=np.int64)
    position[original] = np.arange(n)
    cols, rows = pairs_of(rowptr, truth_idx)
    new_rowptr, new_idx = csr_from_pairs(len(rowptr) - 1, cols, position[rows])
    return new_rowptr, new_idx, sums32[original], original


def forward_lists(rowptr, truth_idx, n):
    """(row_start int64[n + 1], columns int64[nnz]): the columns of every row, ascending, row after row."""
    cols, rows = pairs_of(rowptr, truth_idx)
    order = np.lexsort((cols, rows))
    starts = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=starts[1:])
    return starts, cols[order]


def hash_groups(rowptr, truth_idx, sums32, hash_bits=0):
    """(the hash groups of duplicate_ranks_rule: lists of rows, ascending; the column list of every row as bytes)."""
    sums32 = np.ascontiguousarray(sums32, dtype=np.float32)
    n = sums32.shape[0]
    starts, cols = forward_lists(rowptr, truth_idx, n)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(starts))
    a, b = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        g = cols.astype(np.uint64)
        np.add.at(a, rows, mix64(g + np.uint64(0x9e3779b97f4a7c15)))
        np.add.at(b, rows, mix64(g * np.uint64(0xd6e8feb86659fd93) + np.uint64(0x2545f4914f6cdd1d)))
    if hash_bits and hash_bits < 64:
        mask = np.uint64((1 << hash_bits) - 1)
        a, b = a & mask, b & mask
    lists = [cols[starts[t]:starts[t + 1]].tobytes() for t in range(n)]
    groups = {}
    for t, key in enumerate(zip(a.tolist(), b.tolist(), sums32.view(np.uint32).tolist())):
        groups.setdefault(key, []).append(t)
    return list(groups.values()), lists


def duplicate_ranks_rule(rowptr, truth_idx, sums32, hash_bits=0):
    """uint16[N]: a hash group = the rows with equal (hash a, hash b, sums32 bits), the hashes being the sums of the mix64
    images of a row's columns, cut to their low `hash_bits` bits (0: all).  The group's first row is its largest.  Every
    other member is compared with THAT row's column list only; one that differs keeps rank 0 even when it equals another
    member.  A verified member's rank = 1 + the verified members with a larger row index, at most 65,535."""
    rank = np.zeros(np.asarray(sums32).shape[0], dtype=np.uint16)
    groups, lists = hash_groups(rowptr, truth_idx, sums32, hash_bits)
    for members in groups:
        first, verified = members[-1], 0
        for t in reversed(members[:-1]):
            if lists[t] == lists[first]:
                verified += 1
                rank[t] = min(verified, 65535)
    return rank


def part_edges_problem(sums="equal", full_column=True, seed=7):
    """V = 40 columns over two narrow tiles and a short third one (100 rows).  Column j < 25 holds, in EACH of the three
    tiles, (0, 1, 3, 4, 5)[j % 5] even and (0, 1, 3, 4, 5)[j // 5] odd tile-local rows (the lowest ones) when the
    internal order is the caller's (sums = "equal": all sums32 equal, the order is the stable tie rule alone).  Column 25
    is empty, column 26 holds every row (full_column) or none, columns 27..39 hold random rows of the upper half of every
    tile; rows with no column at all are the rest (without the full column).
    sums: "equal" | "runs" (runs of 5,000 equal values in a shuffled caller order: they straddle both tile boundaries) |
    "signed" (runs, with -0.0, +0.0 and negative values, and a negative idf32: literal_only)."""
    rng = np.random.RandomState(seed)
    n, v, counts = 2 * NARROW + 100, 40, (0, 1, 3, 4, 5)
    cols, rows = [], []
    for j in range(25):
        for first in (0, NARROW, 2 * NARROW):
            local = [2 * i for i in range(counts[j % 5])] + [2 * i + 1 for i in range(counts[j // 5])]
            cols += [j] * len(local)
            rows += [first + r for r in local]
    if full_column:
        cols += [26] * n
        rows += list(range(n))
    for j in range(27, 40):
        for first, size in ((0, NARROW), (NARROW, NARROW), (2 * NARROW, 100)):
            picked = first + size // 2 + rng.choice(size // 2, size=min(size // 2, 1 + 37 * (j - 26)) // 2, replace=False)
            cols += [j] * picked.shape[0]
            rows += picked.tolist()
    rowptr, truth_idx = csr_from_pairs(v, cols, rows)
    idf32 = (1.0 + rng.rand(v)).astype(np.float32)
    if sums == "equal":
        sums32 = np.full(n, 1.5, dtype=np.float32)
    else:
        sums32 = (rng.permutation(n) // 5000).astype(np.float32)
        if sums == "signed":
            sums32 -= 2.0
            zeros = np.nonzero(sums32 == 0)[0]
            sums32[zeros[::2]] = -0.0
            idf32[3] = -0.25
    return rowptr, truth_idx, idf32, sums32, v, n


def twins_problem(seed=11):
    """75,600 rows over 50 columns: 70,000 rows with columns {0, 1, 2} and sums32 1.0 (their ranks saturate), 600 rows with
    {3, 4} and 12.0 that lie across the boundary of tiles 5 and 6 in the internal order, 50 rows with {3, 4} and the next
    float above 12.0 (same set, other bits: no twins of the 600), and 4,950 others whose column sets come from a pool of 60
    and whose sums32 from 12 values (so that they have twins of their own, and share hash groups once the hashes are cut):
    3,428 of them below 12.0, the rest above.  Caller order: shuffled."""
    rng = np.random.RandomState(seed)
    pool = [tuple(sorted(rng.choice(np.arange(5, 50), size=rng.randint(1, 6), replace=False).tolist())) for _ in range(60)]
    sets, sums = [(0, 1, 2)] * 70000 + [(3, 4)] * 650, [1.0] * 70000 + [12.0] * 600 + [float(np.nextafter(np.float32(12), np.float32(13)))] * 50
    low, high = np.arange(2, 8, dtype=np.float64), np.arange(14, 20, dtype=np.float64)
    for i in range(4950):
        sets.append(pool[rng.randint(60)])
        sums.append(float(rng.choice(low if i < 3428 else high)))
    n = len(sets)
    shuffle = rng.permutation(n)
    cols, rows = [], []
    for row, which in enumerate(shuffle):
        cols += sets[which]
        rows += [row] * len(sets[which])
    rowptr, truth_idx = csr_from_pairs(50, cols, rows)
    sums32 = np.asarray(sums, dtype=np.float32)[shuffle]
    idf32 = np.full(50, 0.5, dtype=np.float32)
    return rowptr, truth_idx, idf32, sums32, 50, n


def wide_columns_problem(seed=3):
    """V = 70,000 > 65,536 columns over N = 2,000 rows: the forward index holds int32 columns."""
    rng = np.random.RandomState(seed)
    v, n = 70000, 2000
    cols = np.concatenate((rng.randint(0, v, 30000), [v - 1, v - 1, 65535, 65536, 65537]))
    rows = np.concatenate((rng.randint(0, n, 30000), [0, n - 1, 5, 5, 5]))
    pairs = np.unique(cols.astype(np.int64) * n + rows)
    rowptr, truth_idx = csr_from_pairs(v, pairs // n, pairs % n)
    idf32 = (0.5 + rng.rand(v)).astype(np.float32)
    sums32 = (rng.rand(n) * 40).astype(np.float32)
    return rowptr, truth_idx, idf32, sums32, v, n


def refused_inputs():
    """name -> (rowptr, truth_idx, idf32, sums32, V, N, what the message holds): inputs the validation stage rejects."""
    idf32, sums32 = np.ones(3, dtype=np.float32), np.ones(6, dtype=np.float32)
    make = lambda rowptr, idx: (np.asarray(rowptr, dtype=np.int64), np.asarray(idx, dtype=np.int32), idf32, sums32, 3, 6)
    return {"repeated": make([0, 2, 5, 6], [0, 1, 2, 2, 4, 5]) + (b"column 1 is not strictly ascending",),
            "descending": make([0, 2, 5, 6], [0, 1, 4, 3, 5, 5]) + (b"column 1 is not strictly ascending",),
            "row_equal_to_n": make([0, 2, 5, 6], [0, 1, 2, 3, 4, 6]) + (b"column 2 is not strictly ascending",),
            "rowptr_not_monotone": make([0, 3, 2, 6], [0, 1, 2, 3, 4, 5]) + (b"rowptr not monotone at column 1",)}


# ---- the whole image, restated ---------------------------------------------------------------------------------------
SIGNATURE_BITS, RECORD_WORDS = 128, 8


def idf_totals(rowptr, truth_idx, idf32, n):
    """float64[n]: the sum of the idf32 of every row's columns, added one by one in ascending column order."""
    starts, cols = forward_lists(rowptr, truth_idx, n)
    values = np.asarray(idf32, dtype=np.float32).astype(np.float64)[cols]
    totals, lengths = np.zeros(n, dtype=np.float64), np.diff(starts)
    for k in range(int(lengths.max()) if n else 0):           # the k-th column of every row that has one
        active = np.nonzero(lengths > k)[0]
        totals[active] = totals[active] + values[starts[active] + k]
    return totals


def true_sums(rowptr, truth_idx, idf32, n):
    """float32[n]: the reference's sums32, a sequential float32 sum over a row's columns in ascending order."""
    starts, cols = forward_lists(rowptr, truth_idx, n)
    values = np.asarray(idf32, dtype=np.float32)[cols]
    sums, lengths = np.zeros(n, dtype=np.float32), np.diff(starts)
    for k in range(int(lengths.max()) if n else 0):
        active = np.nonzero(lengths > k)[0]
        sums[active] = sums[active] + values[starts[active] + k]
    return sums


def signature_columns(rowptr, n):
    """int8[V]: the bit of the up to 128 longest lists, ties to the lower column, cut at the first with length * 256 < N."""
    lengths = np.diff(np.asarray(rowptr, dtype=np.int64))
    sig_column = np.full(lengths.shape[0], -1, dtype=np.int8)
    by_length = sorted(range(lengths.shape[0]), key=lambda g: (-int(lengths[g]), g))
    for bit, g in enumerate(by_length[:SIGNATURE_BITS]):
        if int(lengths[g]) * 256 < n:
            break
        sig_column[g] = bit
    return sig_column


def in_range(values):
    """The build's range test of idf32 and sums32, in float32: 0 <= x < 1e30 (false for a NaN)."""
    values = np.asarray(values, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return (values >= np.float32(0)) & (values < np.float32(1e30))


def literal_only_rule(rowptr, truth_idx, idf32, sums32):
    """1 when any idf32 or sums32 is outside [0, 1e30) or any row's sums32 lies below its idf total * (1 - 1e-4)."""
    sums32 = np.asarray(sums32, dtype=np.float32)
    totals = idf_totals(rowptr, truth_idx, idf32, sums32.shape[0])
    with np.errstate(invalid="ignore"):
        low = sums32.astype(np.float64) < totals * (1.0 - 1e-4)
    return int(not in_range(idf32).all() or not in_range(sums32).all() or bool(low.any()))


def tile_bounds_rule(sums_internal, tile_rows):
    """(tile_sums_min, tile_sums_max, sums_min): the host's loop, literally.  A tile starts from its first row and takes
    another row on a strict < (>) only: the first of equal values stays (-0.0 next to +0.0), a NaN is never taken, and a
    NaN the tile starts from is never left."""
    n = sums_internal.shape[0]
    values = sums_internal.astype(np.float64).tolist()            # exact, and a NaN stays a NaN
    n_tiles = (n + tile_rows - 1) // tile_rows
    low, high = np.zeros(n_tiles, dtype=np.float32), np.zeros(n_tiles, dtype=np.float32)
    for b in range(n_tiles):
        first = b * tile_rows
        lowest = highest = first
        for t in range(first + 1, min(n, first + tile_rows)):
            if values[t] < values[lowest]:
                lowest = t
            if values[highest] < values[t]:
                highest = t
        low[b], high[b] = sums_internal[lowest], sums_internal[highest]   # the row's own bits
    sums_min = sums_internal[0:1].copy()
    for b in range(n_tiles):
        if float(low[b]) < float(sums_min[0]):
            sums_min[0] = low[b]
    return low, high, sums_min


def expected_image(rowptr, truth_idx, idf32, sums32, tile_rows, sort_rows=True, hash_bits=0):
    """The image of TruthIndex.image() -- every array of IMAGE_ARRAYS, every scalar of IMAGE_SCALARS -- from the documented
    rule, in NumPy and Python loops.  For small inputs."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    idf32 = np.ascontiguousarray(idf32, dtype=np.float32)
    sums32 = np.ascontiguousarray(sums32, dtype=np.float32)
    v, n, nnz = rowptr.shape[0] - 1, sums32.shape[0], int(rowptr[-1])
    assert tile_rows > 0 and tile_rows % 2 == 0
    n_tiles = (n + tile_rows - 1) // tile_rows
    # internal order: stable by the order key; record words 4 and 6; sums32 padded by 8 zeros
    p_rowptr, p_idx, p_sums, original = internal_csr(rowptr, truth_idx, sums32, sort_rows)
    records = np.zeros((n, RECORD_WORDS), dtype=np.uint32)
    records[:, 4] = p_sums.view(np.uint32)
    records[:, 5] = duplicate_ranks_rule(p_rowptr, p_idx, p_sums, hash_bits)
    records[:, 6] = original
    # forward index
    starts, forward = forward_lists(p_rowptr, p_idx, n)
    wide_cols = v > 65536
    # signature: words 0..3
    sig_column = signature_columns(rowptr, n)
    cols, rows = pairs_of(p_rowptr, p_idx)
    for g, t in zip(cols.tolist(), rows.tolist()):
        bit = int(sig_column[g])
        if bit >= 0:
            records[t, bit >> 5] |= np.uint32(1 << (bit & 31))
    # quads of every (column, tile) cell, col_ptr: their exclusive sum, column after column, with every column's end
    tile, local = rows // tile_rows, rows % tile_rows
    even, odd = np.zeros((v, n_tiles), dtype=np.int64), np.zeros((v, n_tiles), dtype=np.int64)
    np.add.at(even, (cols[local % 2 == 0], tile[local % 2 == 0]), 1)
    np.add.at(odd, (cols[local % 2 == 1], tile[local % 2 == 1]), 1)
    quads = (even + 3) // 4 + (odd + 3) // 4
    n_quads = int(quads.sum())
    before = np.concatenate(([0], np.cumsum(quads.reshape(-1))))
    col_ptr = np.empty((v, n_tiles + 1), dtype=np.uint32)
    col_ptr[:, :n_tiles] = before[:-1].reshape(v, n_tiles)
    col_ptr[:, n_tiles] = before[n_tiles::n_tiles][:v] if n_tiles else 0
    # postings of every cell: even rows, padding, odd rows, padding
    postings, posting_sums = np.zeros(4 * n_quads, dtype=np.uint16), np.zeros(4 * n_quads, dtype=np.uint16)
    for g in np.nonzero(np.diff(p_rowptr))[0].tolist():
        mine = p_idx[p_rowptr[g]:p_rowptr[g + 1]].astype(np.int64)          # ascending
        for cell in np.split(mine, np.nonzero(np.diff(mine // tile_rows))[0] + 1):     # the rows of one tile
            b = int(cell[0]) // tile_rows
            at = 4 * int(col_ptr[g, b])
            for parity in (0, 1):
                part = [t for t in cell.tolist() if (t - b * tile_rows) % 2 == parity]
                for t in part:
                    postings[at] = (parity << 15) | ((t - b * tile_rows) >> 1)
                    posting_sums[at] = records[t, 0] & 0xffff
                    at += 1
                for _ in range(-len(part) % 4):
                    postings[at] = (parity << 15) | (tile_rows // 2)
                    at += 1
            assert at == 4 * int(col_ptr[g, b + 1])
    tile_min, tile_max, sums_min = tile_bounds_rule(p_sums, tile_rows)
    return {"col_ptr": col_ptr, "postings": postings, "posting_sums": posting_sums, "records": records,
            "sums32": np.concatenate((p_sums, np.zeros(8, dtype=np.float32))), "tile_sums_min": tile_min,
            "tile_sums_max": tile_max, "sig_column": sig_column, "row_start": starts.astype(np.uint32),
            "row_cols": forward.astype(np.int32 if wide_cols else np.uint16), "idf32": idf32.copy(),
            "n_tiles": n_tiles, "n_quads": n_quads, "sums_min_bits": int(sums_min.view(np.uint32)[0]),
            "literal_only": literal_only_rule(rowptr, truth_idx, idf32, sums32), "rows_sorted": int(bool(sort_rows)),
            "row_start_bytes": 4, "row_cols_bytes": 4 if wide_cols else 2, "tile_rows": tile_rows}


def fnv1a(array):
    """FNV-1a, 64 bits, over the bytes of an array."""
    h = 0xcbf29ce484222325
    for byte in np.ascontiguousarray(array).tobytes():
        h = ((h ^ byte) * 0x100000001b3) & 0xffffffffffffffff
    return h


def image_digest(image):
    """The eight words of ds_index_image_digest from an image: col_ptr; postings; posting_sums; records; the tile minima ^
    the tile maxima ^ sums32 without its padding; sig_column ^ the 64-bit row starts (none here) ^ the 32-bit row starts
    ^ the int32 columns ^ the uint16 columns (one of the two is empty); n_quads; literal_only."""
    n = image["records"].shape[0]
    empty = fnv1a(np.zeros(0, dtype=np.uint8))
    assert image["row_start_bytes"] == 4
    wide, narrow = (fnv1a(image["row_cols"]), empty) if image["row_cols_bytes"] == 4 else (empty, fnv1a(image["row_cols"]))
    return [fnv1a(image["col_ptr"]), fnv1a(image["postings"]), fnv1a(image["posting_sums"]), fnv1a(image["records"]),
            fnv1a(image["tile_sums_min"]) ^ fnv1a(image["tile_sums_max"]) ^ fnv1a(image["sums32"][:n]),
            fnv1a(image["sig_column"]) ^ empty ^ fnv1a(image["row_start"]) ^ wide ^ narrow,
            image["n_quads"], image["literal_only"]]


# ---- generated problems ----------------------------------------------------------------------------------------------
SHAPES = ("random", "twins", "single", "dense", "sparse")
SUMS = ("true", "equal", "few", "specials", "edge_low")
SPECIAL_BITS = {"+nan": 0x7fc00000, "-nan": 0xffc00000, "+inf": 0x7f800000, "-inf": 0xff800000, "-0.0": 0x80000000,
                "+0.0": 0x00000000, "denormal": 0x00011704, "negative": 0xc0600000, "1e30": 0x7149f2ca,
                "below_1e30": 0x7149f2c9}


def row_columns_of(rng, n_rows, n_columns, shape):
    """The columns of every row, ascending: the four shapes of test_gpu_property._problem (the same draws from rng, in
    the same order) and "sparse", where four rows of five hold no column at all, the first and last two among them."""
    if shape == "twins":                       # a handful of distinct column sets, each repeated many times
        kinds = [np.unique(rng.randint(0, n_columns, rng.randint(1, 9))) for _ in range(rng.randint(1, 6))]
        return [kinds[rng.randint(len(kinds))] for _ in range(n_rows)]
    if shape == "single":                      # most rows hold one column: massive ties
        return [np.array([rng.randint(n_columns)]) if rng.rand() < 0.9 else np.unique(rng.randint(0, n_columns, 3))
                for _ in range(n_rows)]
    if shape == "dense":                       # a few columns present in most rows (signature columns) + a sparse tail
        heavy = min(n_columns, 6)
        return [np.unique(np.concatenate((np.nonzero(rng.rand(heavy) < 0.6)[0], rng.randint(0, n_columns, rng.randint(1, 5)))))
                for _ in range(n_rows)]
    if shape == "sparse":
        rows = [np.unique(rng.randint(0, n_columns, rng.randint(1, 6))) if rng.rand() < 0.2 else np.zeros(0, dtype=np.int64)
                for _ in range(n_rows)]
        for t in (0, 1, n_rows - 2, n_rows - 1):
            rows[min(max(t, 0), n_rows - 1)] = np.zeros(0, dtype=np.int64)
        return rows
    assert shape == "random", shape
    return [np.unique(rng.randint(0, n_columns, rng.randint(1, 14))) for _ in range(n_rows)]


@functools.lru_cache(maxsize=2)
def _generated_rows(seed, n_rows, n_columns, shape):
    """(the columns of every row, the state of the generator behind them): made once for a problem and its queries."""
    rng = np.random.RandomState(seed)
    return row_columns_of(rng, n_rows, n_columns, shape), rng.get_state()


def csr_and_idf(row_columns, n_columns):
    """(rowptr, truth_idx, idf64) of test_gpu_property._problem: idf = log(N / df), the largest of them for an empty column."""
    n = len(row_columns)
    rows = np.concatenate([np.full(len(c), t, dtype=np.int64) for t, c in enumerate(row_columns)])
    cols = np.concatenate(row_columns).astype(np.int64)
    order = np.argsort(cols, kind="stable")
    df = np.bincount(cols, minlength=n_columns)
    rowptr = np.concatenate(([0], np.cumsum(df))).astype(np.int64)
    idf64 = np.log(n / np.maximum(df, 1))
    idf64[df == 0] = idf64.max() if (df > 0).any() else 1.0
    return rowptr, rows[order].astype(np.int32), idf64


def float32_around(bound):
    """(the largest float32 below the float64 `bound`, the smallest float32 not below it)."""
    at = np.float32(bound)
    while float(at) >= bound:
        at = np.nextafter(at, np.float32(-np.inf))
    return at, np.nextafter(at, np.float32(np.inf))


def adversarial_problem(seed, n_rows, n_columns, shape, sums):
    """(rowptr, truth_idx, idf32, sums32, V, N) of a generated index; shape: one of SHAPES, sums: one of SUMS --
    "true": the sequential float32 sum of the row's idf32; "equal": 1.5 everywhere; "few": three values; "specials": true
    sums with up to ten rows replaced by the values of SPECIAL_BITS; "edge_low": true sums with one row just under its
    idf total * (1 - 1e-4) and another at the first float32 not under it."""
    assert shape in SHAPES and sums in SUMS, (shape, sums)
    rowptr, truth_idx, idf64 = csr_and_idf(_generated_rows(seed, n_rows, n_columns, shape)[0], n_columns)
    idf32 = idf64.astype(np.float32)
    sums32 = true_sums(rowptr, truth_idx, idf32, n_rows)
    rng = np.random.RandomState(seed ^ 0x5eed)      # the draws of the rows stay those of test_gpu_property._problem
    if sums == "equal":
        sums32 = np.full(n_rows, 1.5, dtype=np.float32)
    elif sums == "few":
        sums32 = rng.choice(np.array([0.25, 1.5, 7.0], dtype=np.float32), n_rows)
    elif sums == "specials":
        picked = rng.choice(n_rows, size=min(n_rows, len(SPECIAL_BITS)), replace=False)
        values = np.array(list(SPECIAL_BITS.values()), dtype=np.uint32)[rng.permutation(len(SPECIAL_BITS))]
        sums32[picked] = values[:picked.shape[0]].view(np.float32)
    elif sums == "edge_low":
        totals = idf_totals(rowptr, truth_idx, idf32, n_rows)
        positive = np.nonzero(totals > 0)[0]
        picked = rng.choice(positive, size=min(2, positive.shape[0]), replace=False)
        for which, t in enumerate(picked.tolist()):
            sums32[t] = float32_around(totals[t] * (1.0 - 1e-4))[which]
    return rowptr, truth_idx, idf32, sums32, n_columns, n_rows


def adversarial_queries(seed, n_rows, n_columns, shape, n_queries=12):
    """(q_rowptr, q_cols, q_maxint) for adversarial_problem(seed, ..., shape, "true"): the queries of
    test_gpu_property._problem (a truth row, 0..128 random columns, every column, a truth row + noise, a few columns)."""
    row_columns, state = _generated_rows(seed, n_rows, n_columns, shape)
    rng = np.random.RandomState()
    rng.set_state(state)                              # the queries are drawn behind the rows, as in _problem
    idf64 = csr_and_idf(row_columns, n_columns)[2]
    idf32 = idf64.astype(np.float32)
    q_cols, q_maxint = [], []
    for _ in range(n_queries):
        kind = rng.randint(5)
        if kind == 0:
            c = row_columns[rng.randint(n_rows)]
        elif kind == 1:
            c = np.unique(rng.randint(0, n_columns, rng.randint(0, min(129, n_columns + 1))))
        elif kind == 2:
            c = np.arange(min(n_columns, 128))
        elif kind == 3:
            c = np.unique(np.concatenate((row_columns[rng.randint(n_rows)], rng.randint(0, n_columns, 2))))
        else:
            c = np.unique(rng.randint(0, n_columns, rng.randint(1, 30)))
        c = c[idf32[c] != 0].astype(np.int64)
        q_cols.append(c)
        total = 0.0
        for value in idf64[c]:
            total = total + float(value)
        q_maxint.append(total)
    q_rowptr = np.concatenate(([0], np.cumsum([len(c) for c in q_cols]))).astype(np.int64)
    flat = np.concatenate(q_cols).astype(np.int32) if q_rowptr[-1] else np.zeros(0, np.int32)
    return q_rowptr, flat, np.array(q_maxint, dtype=np.float64)


# ---- named edge problems ---------------------------------------------------------------------------------------------
ROWS_AT = (2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 65535, 65536, 65537)
COLUMNS_AT = (2, 127, 128, 129, 255, 256, 257, 65535, 65536, 65537)
POSTINGS_AT = (2047, 2048, 2049, 4096)
NO_POSTINGS = (5, 64, 300)
HASH_BITS = (1, 3, 9)


def bits_of(count):
    """ds_index_build.hip: the bits that hold every value below count (at least 1)."""
    bits = 1
    while (1 << bits) < count:
        bits += 1
    return bits


def sort_passes(count):
    """8-bit digit passes of the device build's sort over values below count."""
    return (bits_of(count) + 7) // 8


def _with_true_sums(n_columns, n_rows, cols, rows, rng):
    rowptr, truth_idx = csr_from_pairs(n_columns, cols, rows)
    idf32 = (0.5 + rng.rand(n_columns)).astype(np.float32)
    return rowptr, truth_idx, idf32, true_sums(rowptr, truth_idx, idf32, n_rows), n_columns, n_rows


def one():
    """N = V = nnz = 1."""
    half = np.array([0.5], dtype=np.float32)
    return np.array([0, 1], dtype=np.int64), np.array([0], dtype=np.int32), half, half.copy(), 1, 1


def no_postings(n, seed=5, values=(0.0, 1.0, 2.5)):
    """n rows, three columns, no posting: every row an empty-set twin of the rows with its sums32 value (three values)."""
    rng = np.random.RandomState(seed)
    sums32 = rng.choice(np.array(values, dtype=np.float32), n)
    return np.zeros(4, dtype=np.int64), np.zeros(0, dtype=np.int32), np.ones(3, dtype=np.float32), sums32, 3, n


def rows_at(n, seed=21):
    """n rows over nine columns, each column in a row with probability 1 / 3; true sums."""
    rng = np.random.RandomState(seed)
    cols, rows = np.nonzero(rng.rand(9, n) < 1.0 / 3.0)
    return _with_true_sums(9, n, cols, rows, rng)


def columns_at(v, seed=22):
    """500 rows over v columns.  Five long lists (100..300 rows); then 140 columns (all of them when v < 145) with two rows
    each -- the shortest list that earns a signature bit at 500 rows (2 * 256 >= 500) -- among them columns 0, v - 1,
    65535 and 65536 where they exist, so the 128 bits run out inside a tie; 200 more columns with one row; the rest empty."""
    rng = np.random.RandomState(seed)
    n = 500
    must = np.unique([c for c in (0, v - 1, 65535, 65536) if c < v])
    others = rng.permutation(np.setdiff1d(np.arange(v), must))
    tied = np.concatenate((must, others[:max(0, min(v, 140) - must.shape[0])]))
    others = others[tied.shape[0] - must.shape[0]:]
    lengths = np.zeros(v, dtype=np.int64)
    lengths[tied] = 2
    lengths[others[:5]] = 100 + 50 * np.arange(min(5, others.shape[0]))
    lengths[others[5:205]] = 1
    cols, rows = [], []
    for g in np.nonzero(lengths)[0].tolist():
        cols += [g] * int(lengths[g])
        rows += rng.choice(n, size=int(lengths[g]), replace=False).tolist()
    return _with_true_sums(v, n, cols, rows, rng)


def postings_at(m, seed=23):
    """Exactly m postings: m distinct cells of 700 rows x 11 columns; true sums."""
    rng = np.random.RandomState(seed)
    cells = rng.choice(700 * 11, size=m, replace=False)
    return _with_true_sums(11, 700, cells // 700, cells % 700, rng)


def tile_edge_rows(t):
    return (t - 1, t, t + 1, 2 * t, 2 * t + 1)


def tile_edges(n, t, seed=24):
    """n rows around tiles of t rows, in an internal order that is the caller's (every sums32 is 1.0: column 0, idf 1.0,
    holds every row; the other columns have idf 0.0).  Column 1 holds the last row of tile 0 and the first of tile 1
    (those of them that exist), column 2 one row in a hundred."""
    rng = np.random.RandomState(seed)
    boundary = [r for r in (t - 1, t) if r < n]
    some = np.nonzero(rng.rand(n) < 0.01)[0]
    rowptr, truth_idx = csr_from_pairs(3, [0] * n + [1] * len(boundary) + [2] * some.shape[0],
                                       list(range(n)) + boundary + some.tolist())
    idf32 = np.array([1.0, 0.0, 0.0], dtype=np.float32)
    return rowptr, truth_idx, idf32, true_sums(rowptr, truth_idx, idf32, n), 3, n


def nan_tiles(t, seed=25):
    """t + 5 rows over six columns; true sums but for twelve rows.  Sorted, internal row 0 is the -NaN and the whole last
    tile (five rows) +NaNs of five payloads.  In the caller's order (DS_SORT_ROWS=0) tile 1 starts with a NaN and holds
    another, tile 0 holds three NaNs and the -NaN past its first row, and its smallest values are, in this order,
    -0.0, +0.0, -0.0, +0.0 (rows 10, 20, 30, 40)."""
    rng = np.random.RandomState(seed)
    n = t + 5
    assert t >= 64
    cols, rows = np.nonzero(rng.rand(6, n) < 0.4)
    rowptr, truth_idx, idf32, sums32, _, _ = _with_true_sums(6, n, cols, rows, rng)
    sums32 = np.maximum(sums32, np.float32(0.125))                 # the zeros below are the smallest values
    bits = sums32.view(np.uint32)
    for row, value in zip((t, t + 2, 5, t // 2, t - 3), range(5)):
        bits[row] = 0x7fc00000 + value
    bits[t // 3] = 0xffc00000
    bits[[10, 30]], bits[[20, 40]] = 0x80000000, 0x00000000
    return rowptr, truth_idx, idf32, sums32, 6, n


def one_bad_row(bad_row=4999, seed=26):
    """5,000 rows over 50 columns with true sums, but row bad_row: the largest float32 under its idf total * (1 - 1e-4)."""
    rng = np.random.RandomState(seed)
    n = 5000
    cols, rows = np.nonzero(rng.rand(50, n) < 0.08)
    cols, rows = np.concatenate((cols, [7, 31])), np.concatenate((rows, [bad_row, bad_row]))
    pairs = np.unique(cols.astype(np.int64) * n + rows)
    rowptr, truth_idx, idf32, sums32, _, _ = _with_true_sums(50, n, pairs // n, pairs % n, rng)
    sums32[bad_row] = float32_around(idf_totals(rowptr, truth_idx, idf32, n)[bad_row] * (1.0 - 1e-4))[0]
    return rowptr, truth_idx, idf32, sums32, 50, n


def stray_largest(hash_bits, seed=27):
    """40 hash groups under hashes cut to hash_bits bits, one per sums32 value (1.0, 2.0, ...), the rows of the groups
    interleaved in the caller's order.  Every group is made of two column sets S1 != S2 whose cut hashes collide.  Even
    groups: S1 x 4, then S2 -- the group's largest row is no twin of the rest, and every rank is 0.  Odd groups: S2, S2, S1,
    S1, S2 -- the largest row has two twins, the S1 rows keep rank 0.  Under whole hashes every set has its own ranks."""
    rng = np.random.RandomState(seed)
    v, groups = 40, 40
    sets = [(a,) for a in range(v)] + [(a, b) for a in range(v) for b in range(a + 1, v)] + \
           [(a, b, c) for a in range(v) for b in range(a + 1, v) for c in range(b + 1, v)]
    mask = np.uint64((1 << hash_bits) - 1)
    with np.errstate(over="ignore"):
        g = np.arange(v, dtype=np.uint64)
        image_a, image_b = mix64(g + np.uint64(0x9e3779b97f4a7c15)), mix64(g * np.uint64(0xd6e8feb86659fd93) + np.uint64(0x2545f4914f6cdd1d))
        seen, pairs = {}, []
        for which in rng.permutation(len(sets)).tolist():
            key = (int(image_a[list(sets[which])].sum() & mask), int(image_b[list(sets[which])].sum() & mask))
            if key in seen:
                pairs.append((sets[seen.pop(key)], sets[which]))
                if len(pairs) == groups:
                    break
            else:
                seen[key] = which
    assert len(pairs) == groups
    cols, rows, sums = [], [], []
    for position in range(5):
        for group, (s1, s2) in enumerate(pairs):
            held = ((s1, s1, s1, s1, s2) if group % 2 == 0 else (s2, s2, s1, s1, s2))[position]
            cols += held
            rows += [len(sums)] * len(held)
            sums.append(1.0 + group)
    rowptr, truth_idx = csr_from_pairs(v, cols, rows)
    return rowptr, truth_idx, np.full(v, 0.25, dtype=np.float32), np.asarray(sums, dtype=np.float32), v, len(sums)


def named_problems(max_rows=None, tile=NARROW):
    """name -> a function that makes the problem, for every named edge problem of up to max_rows rows."""
    made = {"one": one}
    made.update({f"no_postings[{n}]": (lambda n=n: no_postings(n)) for n in NO_POSTINGS})
    made.update({f"rows_at[{n}]": (lambda n=n: rows_at(n)) for n in ROWS_AT})
    made.update({f"columns_at[{v}]": (lambda v=v: columns_at(v)) for v in COLUMNS_AT})
    made.update({f"postings_at[{m}]": (lambda m=m: postings_at(m)) for m in POSTINGS_AT})
    made.update({f"tile_edges[{n}]": (lambda n=n: tile_edges(n, tile)) for n in tile_edge_rows(tile)})
    made.update({"nan_tiles": lambda: nan_tiles(tile), "nan_tiles[64]": lambda: nan_tiles(64)})
    made.update({f"one_bad_row[{row}]": (lambda row=row: one_bad_row(row)) for row in (4999, 2500)})
    made.update({f"stray_largest[{b}]": (lambda b=b: stray_largest(b)) for b in HASH_BITS})
    rows_of = {"one": 1, "nan_tiles": tile + 5, "nan_tiles[64]": 69}
    def n_rows(name):
        kind, _, argument = name.partition("[")
        if name in rows_of:
            return rows_of[name]
        return {"no_postings": lambda a: a, "rows_at": lambda a: a, "columns_at": lambda a: 500, "postings_at": lambda a: 700,
                "tile_edges": lambda a: a, "one_bad_row": lambda a: 5000, "stray_largest": lambda a: 200}[kind](int(argument[:-1]))
    return {name: make for name, make in made.items() if max_rows is None or n_rows(name) <= max_rows}
