"""Guards for the two GPU-side failures of round 2 (causes: profiles/r03_failure_causes.md).

(a) r02t / r02u -- the collect sweep's one-compare row test let through (i) padding / idle-lane entries, whose local row
    lies behind the tile (an out-of-range gather in the refinement: the abort), and (ii) the SECOND posting of a row whose
    score another lane had already taken (score 0 + the skipped columns' mass >= need: the row was appended twice and came
    out twice -- rows "not strictly descending").  The guard runs the fast kernel of a -DDS_BOUNDS_CHECK build (every
    data-dependent global index checked, first violation recorded in ds_jaccard_sync stats[28..30]) on an index built so
    that most candidate rows receive postings from two or three essential columns inside one sparse tile.
(b) the epoch redo -- an overflow of the candidate buffer inside an epoch's later tiles processes the epoch again under a
    tighter threshold; round 2's first version reset its retry counter on the epoch's first (successful) tile and never
    ended.  `sparse_redos` (stats[31]) now counts the redos: one scenario must redo and succeed, one (a thousand non-twin
    rows tied within 1e-6) must give up after its retries and hand the query to the literal kernel.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import jaccard_cases
from jaccard_cases import build_index

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NARROW_TILE = jaccard_cases.GEOMETRY["narrow"]["tile_rows"]
# The problems are functions of the geometry in jaccard_cases.py (second_posting_problem, descending_epochs_problem,
# redo_problem); this module runs them narrow, test_gpu_jaccard_geometries.py in both geometries.

_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import doppel_speller_amd as ds
from oracle import oracle
import jaccard_cases
oracle.build()
if %(arrays_file)r:      # the caller built the problem and its expected rows already
    with np.load(%(arrays_file)r) as saved:
        rowptr, truth_idx, idf32, sums32, q_rowptr, q_cols, q_maxint, expected = (saved[name] for name in (
            "rowptr", "truth_idx", "idf32", "sums32", "q_rowptr", "q_cols", "q_maxint", "expected"))
    k = expected.shape[1]
else:
    rowptr, truth_idx, idf32, sums32, q_rowptr, q_cols, q_maxint, k = jaccard_cases.arrays(getattr(jaccard_cases, %(problem)r)(%(geometry)r))
    expected = oracle.jaccard_topk(rowptr, truth_idx, idf32, sums32, q_rowptr, q_cols, q_maxint, k)
index = ds.TruthIndex(rowptr, truth_idx, idf32, sums32)
rows = index.top_k(q_rowptr, q_cols, q_maxint, k)
d_rowptr, d_cols, d_maxint = (ds._lib.DeviceArray.from_host(x) for x in (q_rowptr, q_cols, q_maxint))
d_rows = ds._lib.DeviceArray(rows.shape, np.int32)
index.top_k_device(d_rowptr.ptr, d_cols.ptr, d_maxint.ptr, rows.shape[0], k, d_rows.ptr)
stats = index.sync()
print(json.dumps({"equal": bool(np.array_equal(rows, expected)), "device_equal": bool(np.array_equal(d_rows.to_host(), expected)),
                  "descending": bool((np.diff(rows.astype(np.int64), axis=1) < 0).all()),
                  "bounds_record": [int(x) for x in stats["bounds_record"]], "sparse_tiles": int(stats["sparse_tiles"]),
                  "dense_queries": int(stats["dense_queries"]), "error_queries": int(stats["error_queries"]),
                  "sparse_redos": int(stats["sparse_redos"]), "tiles": int(index.info()["tiles"]),
                  "tile_rows": int(index.info()["tile_rows"]), "status": [int(x) for x in index.status(rows.shape[0])],
                  "library": ds._lib.library_path()}))
"""


def _under_the_bounds_checking_build(problem, geometry="narrow", arrays_file=None):
    """Runs `jaccard_cases.<problem>(geometry)` -- or the arrays and expected rows of `arrays_file` (np.savez) -- through both
    entries of a -DDS_BOUNDS_CHECK build in a fresh process, with the geometry forced."""
    from doppel_speller_amd import _lib
    variant = _lib.build_library(variant="boundscheck")      # built by __graft_entry__.build(); rebuilt here if stale
    env = dict(os.environ, DS_LIBRARY=variant, DS_GEOMETRY=geometry)
    script = _CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests"), "problem": problem, "geometry": geometry,
                       "arrays_file": arrays_file or ""}
    result = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=600)
    assert result.returncode == 0, result.stderr[-3000:]
    outcome = json.loads(result.stdout.strip().splitlines()[-1])
    assert outcome["library"] == variant and outcome["tile_rows"] == jaccard_cases.GEOMETRY[geometry]["tile_rows"]
    return outcome


def test_second_posting_of_a_taken_row_under_the_bounds_checking_build():
    outcome = _under_the_bounds_checking_build("second_posting_problem")
    assert outcome["bounds_record"] == [0, 0, 0], outcome           # no data-dependent global index left its array
    assert outcome["equal"] and outcome["device_equal"] and outcome["descending"], outcome
    assert outcome["sparse_tiles"] > 48 and outcome["dense_queries"] == 0 and outcome["error_queries"] == 0, outcome


def test_descending_epochs_pointer_blocks_under_the_bounds_checking_build():
    outcome = _under_the_bounds_checking_build("descending_epochs_problem")
    assert outcome["tiles"] == 13, outcome
    assert outcome["bounds_record"] == [0, 0, 0], outcome           # list pointers, quads, rows: every index inside its array
    assert outcome["equal"] and outcome["device_equal"] and outcome["descending"], outcome
    assert outcome["sparse_tiles"] > 72 and outcome["error_queries"] == 0, outcome


def _redo_problem(tied):
    return jaccard_cases.arrays(jaccard_cases.redo_problem("narrow", tied))


@pytest.mark.parametrize("tied", [False, True])
def test_candidate_overflow_inside_an_epoch_is_redone_and_counted(oracle, tied, monkeypatch):
    import doppel_speller_amd as ds
    # the scenario places its rows tile by tile: the index keeps the caller's row order (ds_index_create sorts the rows by
    # sums32 otherwise, and a query then starts at the tile of its own sums32)
    monkeypatch.setenv("DS_SORT_ROWS", "0")
    rowptr, truth_idx, idf32, sums32, q_rowptr, q_cols, q_maxint, k = _redo_problem(tied)
    index = ds.TruthIndex(rowptr, truth_idx, idf32, sums32)
    assert index.info()["tile_rows"] == NARROW_TILE
    d_rowptr, d_cols, d_maxint = (ds._lib.DeviceArray.from_host(x) for x in (q_rowptr, q_cols, q_maxint))
    d_rows = ds._lib.DeviceArray((1, k), np.int32)
    index.top_k_device(d_rowptr.ptr, d_cols.ptr, d_maxint.ptr, 1, k, d_rows.ptr)
    stats = index.sync()
    rows = d_rows.to_host()
    expected = oracle.jaccard_topk(rowptr, truth_idx, idf32, sums32, q_rowptr, q_cols, q_maxint, k)
    assert np.array_equal(rows, expected)
    assert stats["error_queries"] == 0
    print("tied" if tied else "distinct", "sparse_redos", stats["sparse_redos"], stats["dense_reasons"])
    if tied:     # no threshold and no admission floor separates a thousand equal rows: the literal kernel answers
        assert stats["sparse_redos"] >= 1 and stats["dense_queries"] == 1
        assert stats["dense_reasons"]["overflow_sparse"] + stats["dense_reasons"]["ties"] == 1
        if stats["dense_reasons"]["overflow_sparse"] == 1:
            # the give-up bound itself (`++sparse_retries > 5`): five redos are counted, the sixth overflow hands the query over.
            # (With the admission floor the bound is a safety net: in a probe with up to 10,000 distinct rows above the cut
            # in one tile, rising or falling with the row index, every query ended after 1..3 redos or as "ties"; none reached it.)
            assert stats["sparse_redos"] == 5, stats["sparse_redos"]
        else:   # the admission floor's check ended it first ("ties": the k best themselves tie at the pivot): fewer redos
            assert stats["sparse_redos"] <= 5, stats["sparse_redos"]
    else:        # the epoch is repeated under the tightened threshold and the admission floor, and fits
        assert 1 <= stats["sparse_redos"] <= 3 and stats["dense_queries"] == 0

    # the same problems with the rows in sums32 order (the default): whatever path they take, the answers are the reference's
    monkeypatch.setenv("DS_SORT_ROWS", "1")
    index = ds.TruthIndex(rowptr, truth_idx, idf32, sums32)
    assert np.array_equal(index.top_k(q_rowptr, q_cols, q_maxint, k), expected)


def test_near_ties_beyond_the_literal_kernels_buffer_are_answered_by_the_row_scan(oracle):
    """More rows within 1e-6 of the k-th value than the literal kernel's LDS buffer holds (3072), none of them twins and
    none k-dominated: the values RISE towards lower row indexes in steps of 6e-14.  The fast kernel hands the query over
    (ties), the streaming selection cannot compact it, and ds_jaccard_sync answers it with the reference's own method --
    the whole float64 jaccard row in an HBM scratch vector (round 2 returned DS_E_INTERNAL here)."""
    import doppel_speller_amd as ds
    n_rows, k = 30000, 10
    band = np.arange(10000, 14500)
    columns = {0: band}
    filler = np.setdiff1d(np.arange(n_rows), band)
    for j, part in enumerate(np.array_split(filler, 50)):
        columns[1 + j] = part
    rowptr, truth_idx, idf32, idf64, _ = build_index(n_rows, columns)
    sums32 = np.full(n_rows, 3.0, dtype=np.float32)
    sums32[band] = (np.float32(2.0).view(np.uint32) + np.arange(band.shape[0], dtype=np.uint32)).view(np.float32)  # one ulp apart, >= the idf of column 0
    q_rowptr = np.array([0, 1], dtype=np.int64)
    q_cols = np.array([0], dtype=np.int32)
    q_maxint = np.array([1000.0])
    expected = oracle.jaccard_topk(rowptr, truth_idx, idf32, sums32, q_rowptr, q_cols, q_maxint, k)
    assert np.array_equal(expected[0], np.arange(14499, 14489, -1))          # the k largest row indexes of the band
    index = ds.TruthIndex(rowptr, truth_idx, idf32, sums32)
    rows = index.top_k(q_rowptr, q_cols, q_maxint, k)
    assert np.array_equal(rows, expected)
    assert index.status(1)[0] == 1          # answered (literal path), not an error
    # the same through the device entry points: the resolution happens inside ds_jaccard_sync
    d_rowptr, d_cols, d_maxint = (ds._lib.DeviceArray.from_host(x) for x in (q_rowptr, q_cols, q_maxint))
    d_rows = ds._lib.DeviceArray((1, k), np.int32)
    index.top_k_device(d_rowptr.ptr, d_cols.ptr, d_maxint.ptr, 1, k, d_rows.ptr)
    stats = index.sync()
    assert stats["error_queries"] == 0 and stats["dense_queries"] == 1 and np.array_equal(d_rows.to_host(), expected)
