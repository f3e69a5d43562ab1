"""Offline model (numpy, CPU) of the skip-set bound: what the sparse sweep traverses and what its row
test lets through, under each query's FINAL threshold, for
    pre = coef * (sums_min + maxint)                               the bound from the index's smallest sums32
    pre = coef * (max(sums_min, cut * maxint) + maxint)            the bound from the band's edge (jaccard <= sums32 / maxint)
Per query: the skipped columns (longest ascending-IDF prefix with mass < pre whose columns all own one of the 128 signature bits),
the postings and posting quads of the ESSENTIAL columns in the band's tiles (a (column, tile) list stores its even and its odd rows
padded to whole quads each), and the rows of those tiles that pass the collect sweep's test -- raw entries -- when a posting carries
    8 signature bits + the 8-bit sums code    (the format until round 6)
    16 membership bits, the tile's smallest sums32 standing in for the row's own.
Rows are in sums32 order, tiles of 12,288 rows (28,672 above 10M rows); fixed-point slack is ignored (it adds a few per cent to
every variant alike).  The thresholds' maturing and the dense start tile are not modelled: they dilute the differences.

usage: sim_skip_bound.py <truth titles> <k> [queries] [query pool]      (~2 min per 100 queries at 500k titles; the pool is the
number of queries the workload is generated with, 100,000 as in bench.py's C2, and the sample is drawn from it)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
from sim_common import code8_lower_bound, index_model  # noqa: E402

N, K = int(sys.argv[1]), int(sys.argv[2])
Q = int(sys.argv[3]) if len(sys.argv) > 3 else 100
POOL = int(sys.argv[4]) if len(sys.argv) > 4 else 100_000
m = index_model(N, POOL)
w, rowptr, tidx, idf32, sums32, TILE, pos, sums_sorted, ntiles, tile_min, tile_max, tile_of_row, tile_min_of_row, df, dense_rank, has_sig = (getattr(m, name) for name in
    "w rowptr tidx idf32 sums32 TILE pos sums_sorted ntiles tile_min tile_max tile_of_row tile_min_of_row df dense_rank has_sig".split())
parity_of_row = (pos % TILE) & 1
sums_lb8 = code8_lower_bound(sums32)
BOUNDS = ("sums_min", "band_edge")
FORMATS = ("8 bits + sums code", "16 membership bits")
skipped_columns = {b: 0 for b in BOUNDS}
postings = {b: 0 for b in BOUNDS}
quads = {b: 0 for b in BOUNDS}
raw = {(b, f): 0 for b in BOUNDS for f in FORMATS}
rng = np.random.RandomState(1)
done = 0
for q in rng.choice(POOL, Q, replace=False):
    cols = np.asarray(w.q_cols[w.q_rowptr[q]:w.q_rowptr[q + 1]])
    n = len(cols)
    if n == 0:
        continue
    maxint = float(w.q_maxint[q])
    o = np.argsort(idf32[cols], kind="stable")
    cs = cols[o]
    idf = idf32[cs].astype(np.float64)
    mass = np.cumsum(idf)
    member = np.zeros((n, N), dtype=bool)                       # member[i, row]: row holds the query's i-th column (ascending idf)
    for i, c in enumerate(cs):
        member[i, tidx[rowptr[c]:rowptr[c + 1]]] = True
    total = (member * idf[:, None]).sum(axis=0)
    jac = total / (sums32.astype(np.float64) + (maxint - total))
    kth = np.partition(jac, N - K)[N - K]
    if kth <= 0:
        continue
    done += 1
    cut = kth - 1e-5
    coef = cut / (1 + cut)
    band_tile = (tile_min * cut <= maxint) & (tile_max >= cut * maxint)
    in_band = band_tile[tile_of_row]
    sig_ok = np.cumprod(has_sig[cs]).astype(bool)
    for bound in BOUNDS:
        floor = float(sums_sorted[0])
        if bound == "band_edge":
            floor = max(floor, cut * maxint * (1.0 - 1e-5))
        ok = (mass < coef * (floor + maxint)) & sig_ok
        skip = int(np.argmin(ok)) if not ok.all() else n
        skipped_columns[bound] += skip
        for i in range(skip, n):                                # the essential columns' lists, tile by tile
            rows = np.nonzero(member[i] & in_band)[0]
            postings[bound] += rows.shape[0]
            per_part = np.bincount(tile_of_row[rows] * 2 + parity_of_row[rows], minlength=2 * ntiles)
            quads[bound] += int(((per_part + 3) // 4).sum())
        s_ess = (member[skip:] * idf[skip:, None]).sum(axis=0)
        touched = (s_ess > 0) & in_band
        for name, bits, lower in ((FORMATS[0], 8, sums_lb8), (FORMATS[1], 16, tile_min_of_row)):
            known = dense_rank[cs[:skip]] < bits                    # membership of these columns travels with the posting
            upper = ((member[:skip] | ~known[:, None]) * idf[:skip, None]).sum(axis=0)
            need = np.maximum(coef * (lower + maxint), coef * (tile_min_of_row + maxint))      # the sums code, never below the tile's gate
            raw[(bound, name)] += int((touched & (s_ess + upper >= need)).sum())
    del member
print(f"N={N} k={K} queries={done}, tiles of {TILE} rows, final thresholds; per query:")
print(f"{'bound':12s}{'skipped columns':>18s}{'essential postings':>20s}{'posting quads':>16s}" + "".join(f"{'raw, ' + f:>28s}" for f in FORMATS))
for bound in BOUNDS:
    print(f"{bound:12s}{skipped_columns[bound] / done:18.2f}{postings[bound] / done:20.0f}{quads[bound] / done:16.0f}" +
          "".join(f"{raw[(bound, f)] / done:28.1f}" for f in FORMATS))
