"""Inputs and restatements for the tests of the device index build (test_index_build_cpu.py, test_gpu_index_build.py).

`duplicate_ranks_rule` restates the duplicate-rank rule of ds::duplicate_ranks in NumPy, with the truncated hashes of
ds_index_build_option("duplicate_hash_bits", b).  `internal_csr` restates the internal row order of ds_index_create
(stable, ascending in its own key of sums32), on which the ranks of an index are computed.  The hand-made CSR and the
twins problem are the inputs of the GPU tests."""
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


def duplicate_ranks_rule(rowptr, truth_idx, sums32, hash_bits=0):
    """uint16[N]: a hash group = the rows with equal (hash a, hash b, sums32 bits), the hashes being the sums of the mix64
    images of a row's columns, cut to their low `hash_bits` bits (0: all).  The group's first row is its largest.  Every
    other member is compared with THAT row's column list only; one that differs keeps rank 0 even when it equals another
    member.  A verified member's rank = 1 + the verified members with a larger row index, at most 65,535."""
    sums32 = np.ascontiguousarray(sums32, dtype=np.float32)
    n = sums32.shape[0]
    cols, rows = pairs_of(rowptr, truth_idx)
    order = np.lexsort((cols, rows))
    cols, rows = cols[order], rows[order]
    starts = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=starts[1:])
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
    rank = np.zeros(n, dtype=np.uint16)
    for members in groups.values():
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
