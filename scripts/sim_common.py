"""What the offline models of the Jaccard kernel share (sim_posting_info.py, sim_skip_bound.py): the synthetic workload in the
kernel's internal row order, its tiles, the signature columns, and the 8-bit sums code a posting carried until round 6."""
import os
import sys
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from doppel_speller_amd import synth  # noqa: E402


def index_model(n_truth, n_queries, seed=20260101):
    """The workload of bench.py (n_truth titles, n_queries queries) with its rows in sums32 order, cut into tiles of 12,288 rows
    (28,672 above 10M rows), and the columns that own one of the 128 signature bits (dense_rank: 0 = the densest column)."""
    tile = 12288 if n_truth <= 10_000_000 else 28672
    w = synth.make_workload(n_truth, n_queries, seed=seed)
    rowptr, tidx, idf32, sums32 = (np.asarray(x) for x in (w.rowptr, w.truth_idx, w.idf32, w.sums32))
    order = np.argsort(sums32, kind="stable")
    pos = np.empty(n_truth, np.int64)
    pos[order] = np.arange(n_truth)
    sums_sorted = sums32[order]
    ntiles = (n_truth + tile - 1) // tile
    tile_min = sums_sorted[np.arange(ntiles) * tile]
    tile_max = sums_sorted[np.minimum(n_truth, (np.arange(ntiles) + 1) * tile) - 1]
    tile_of_row = pos // tile
    df = np.diff(rowptr)
    dense_rank = np.empty(len(df), np.int64)
    dense_rank[np.argsort(-df, kind="stable")] = np.arange(len(df))
    return SimpleNamespace(w=w, rowptr=rowptr, tidx=tidx, idf32=idf32, sums32=sums32, TILE=tile, pos=pos, sums_sorted=sums_sorted,
                           ntiles=ntiles, tile_min=tile_min, tile_max=tile_max, tile_of_row=tile_of_row,
                           tile_min_of_row=tile_min[tile_of_row].astype(np.float64),   # no per-row sums information: the tile's smallest
                           df=df, dense_rank=dense_rank, has_sig=(dense_rank < 128) & (df * 256 >= n_truth))


def code8_lower_bound(x):
    """The 8-bit sums code a posting carried until round 6 (4-bit exponent 2^-3 .. 2^12, 4-bit mantissa, truncated), decoded: a
    lower bound of x."""
    bits = x.astype(np.float32).view(np.uint32)
    exponent = (bits >> 23).astype(np.int64) - 124
    code = np.where(x < 0.125, 0, np.minimum(0xfe, (np.clip(exponent, 0, 15) << 4) | ((bits >> 19) & 0xf)))
    code = np.where(exponent > 15, 0xfe, code)
    out = ((((code >> 4) + 124).astype(np.uint32) << 23) | ((code & 0xf).astype(np.uint32) << 19)).view(np.float32)
    return np.where(code == 0, 0.0, out).astype(np.float64)
