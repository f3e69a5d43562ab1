"""The Jaccard top-k kernel in BOTH of its geometries (narrow: 12,288-row tiles, 256 threads, 768 candidates, epochs of 4
tiles; wide: 28,672 / 512 / 1,472 / 16), on inputs small enough for the suite: every k class and its edges, the counting
instantiations, the sweeps that cross epochs and list-pointer blocks, the epoch redo, and the ledger of hand-overs to the
literal kernel.  The inputs and the proof that each is what it claims are in jaccard_cases.py / test_jaccard_cases_cpu.py;
every comparison here is oracle.jaccard_topk, bit for bit, through the C ABI, on the host entry and on the device entry.

The witnesses are the counters the product build reports through TruthIndex.sync() -- no kernel is changed or mutated.  What
they cannot tell apart is said in the test concerned.  Two things no test here reaches:
  * hand-over reason 1 ("items") is never set by the kernel: every case asserts that it stays 0;
  * the `m > kExactRows` hand-over before the exact stage needs a candidate buffer larger than the exact stage's scratch;
    kExactRows == kCandidates in both shipped geometries, so the site cannot be reached in either.
The per-query counters (sparse_tiles, dense_tiles, selections ...) are summed over the queries the fast kernel ANSWERS; a
query it hands over contributes only its reason, `dense_queries` and -- whatever its redos were -- `sparse_redos`.
"""
import ctypes
import time

import numpy as np
import pytest

import jaccard_cases as jc
from test_gpu_guards import _under_the_bounds_checking_build

pytestmark = pytest.mark.gpu
REASONS = ("shape", "items", "overflow_sparse", "overflow_dense", "ties", "few")


class _Shared:
    """Cases, their indexes (built under DS_GEOMETRY / DS_SORT_ROWS) and the oracle's rows, each made once per module."""

    def __init__(self, oracle):
        self.oracle, self.cases, self.indexes, self.rows = oracle, {}, {}, {}

    def case(self, name, geometry, *args):
        key = (name, geometry) + args
        if key not in self.cases:
            begin = time.perf_counter()
            self.cases[key] = getattr(jc, name)(geometry, *args)
            print("[wall] generation", key, "%.2f s" % (time.perf_counter() - begin))
        return self.cases[key]

    def index(self, name, geometry, *args, sort_rows=True):
        import doppel_speller_amd as ds
        key = (name, geometry) + args + (sort_rows,)
        if key not in self.indexes:
            case = self.case(name, geometry, *args)
            begin = time.perf_counter()
            with pytest.MonkeyPatch.context() as patch:       # the environment is read by ds_index_create only
                patch.setenv("DS_GEOMETRY", geometry)
                patch.setenv("DS_SORT_ROWS", "1" if sort_rows else "0")
                self.indexes[key] = ds.TruthIndex(case["rowptr"], case["truth_idx"], case["idf32"], case["sums32"])
            print("[wall] index build", key, "%.2f s" % (time.perf_counter() - begin))
        index = self.indexes[key]
        assert index.info()["tile_rows"] == jc.GEOMETRY[geometry]["tile_rows"]
        return index

    def expected(self, key, case):
        if key not in self.rows:
            begin = time.perf_counter()
            self.rows[key] = self.oracle.jaccard_topk(*jc.arrays(case))
            print("[wall] oracle", key, "%.2f s" % (time.perf_counter() - begin))
        return self.rows[key]


@pytest.fixture(scope="module")
def shared(oracle):
    return _Shared(oracle)


def _both_entries(index, case, expected):
    """The case through ds_jaccard_topk and through ds_jaccard_topk_device + ds_jaccard_sync: both equal `expected`, both
    keep a consistent ledger.  Returns the device entry's statistics and the status of every query."""
    import doppel_speller_amd as ds
    _, _, _, _, q_rowptr, q_cols, q_maxint, k = jc.arrays(case)
    n_queries = q_maxint.shape[0]
    begin = time.perf_counter()
    rows = index.top_k(q_rowptr, q_cols, q_maxint, k)
    host_stats = index.sync()
    bad = np.nonzero((rows != expected).any(axis=1))[0]
    assert bad.shape[0] == 0, ("host entry", bad[:10], rows[bad[:2]], expected[bad[:2]])
    d_rowptr, d_cols, d_maxint = (ds._lib.DeviceArray.from_host(x) for x in (q_rowptr, q_cols, q_maxint))
    d_rows = ds._lib.DeviceArray((n_queries, k), np.int32)
    index.top_k_device(d_rowptr.ptr, d_cols.ptr, d_maxint.ptr, n_queries, k, d_rows.ptr)
    stats = index.sync()
    status = index.status(n_queries)
    rows = d_rows.to_host()
    print("[wall] both entries %.3f s" % (time.perf_counter() - begin))
    bad = np.nonzero((rows != expected).any(axis=1))[0]
    assert bad.shape[0] == 0, ("device entry", bad[:10], rows[bad[:2]], expected[bad[:2]])
    assert stats["error_queries"] == 0 and host_stats["error_queries"] == 0
    # (the two runs are not compared with each other: whether, and for which of two reasons, a query of tied rows is handed
    # over can depend on the order in which the waves fill the buffer)
    for run in (host_stats, stats):
        assert run["dense_queries"] == sum(run["dense_reasons"].values())
    assert stats["dense_reasons"]["items"] == 0                       # the kernel never sets reason 1
    assert stats["bounds_record"] == [0, 0, 0]
    assert stats["dense_queries"] == int(np.sum(status == 1)) and set(status.tolist()) <= {0, 1}
    return stats, status


def _ledger(stats):
    return {name: stats[name] for name in ("dense_reasons", "sparse_redos", "sparse_tiles", "dense_tiles", "skipped_columns",
                                           "selections", "exact_candidates", "dense_queries", "error_queries", "requested_bytes")}


# ---- k classes and the counting instantiations -------------------------------------------------------------------------
@pytest.mark.parametrize("edge", range(5))
@pytest.mark.parametrize("problem", ["tie_problem", "ragged_problem"])
@pytest.mark.parametrize("geometry", jc.GEOMETRIES)
def test_k_classes_and_their_edges(shared, geometry, problem, edge):
    """k = probe_max_k and probe_max_k + 1 (one sample per thread | two: the <*, true> instantiation), 2 * probe_max_k and
    2 * probe_max_k + 1 (two samples | none: the first threshold comes from a buffer flood and its recovery), and 512, the
    largest k of the selection kernels -- on 3 tiles with 6,000 twins and on 3 tiles plus one row.  An off-by-one in
    launch()'s `second_sample` or in the bootstrap's `k <= (kSecondSample ? 2 : 1) * kProbeMaxK` either takes k-th largest
    of fewer samples than k (a selection of garbage: wrong rows) or skips the bootstrap (still exact): the rows decide."""
    k = jc.k_class_edges(geometry)[edge]
    case = dict(shared.case(problem, geometry), k=k)
    stats, _ = _both_entries(shared.index(problem, geometry), case, shared.expected((problem, geometry, k), case))
    print(geometry, problem, "k", k, _ledger(stats))
    assert stats["selections"] > 0 and stats["dense_tiles"] > 0


@pytest.mark.parametrize("second_sample", [False, True])
@pytest.mark.parametrize("problem", ["tie_problem", "ragged_problem"])
@pytest.mark.parametrize("geometry", jc.GEOMETRIES)
def test_counting_instantiations_return_the_same_rows(shared, geometry, problem, second_sample):
    """ds_index_option("count_bytes", 1) launches ds_jaccard_topk_kernel<true, *> (bench.py's traffic figure); k = 10 and k =
    probe_max_k + 1 take both values of the second template argument.  Same rows, a positive byte count, and none once the
    option is off again."""
    k = jc.probe_max_k(geometry) + 1 if second_sample else 10
    case = dict(shared.case(problem, geometry), k=k)
    index = shared.index(problem, geometry)
    expected = shared.expected((problem, geometry, k), case)
    plain, _ = _both_entries(index, case, expected)
    assert plain["requested_bytes"] == 0
    index.option("count_bytes", 1)
    try:
        counted, _ = _both_entries(index, case, expected)
    finally:
        index.option("count_bytes", 0)
    print(geometry, problem, "k", k, "requested_bytes", counted["requested_bytes"])
    # a query reads at least its own columns, and no more than every posting, pointer and row record a few times over
    assert counted["requested_bytes"] > 4 * case["q_cols"].shape[0]
    again, _ = _both_entries(index, case, expected)
    assert again["requested_bytes"] == 0


# ---- sweeps ------------------------------------------------------------------------------------------------------------------
def _saved(tmp_path_factory, name, case, expected):
    path = str(tmp_path_factory.mktemp("jaccard") / (name + ".npz"))
    np.savez(path, expected=expected, **{key: case[key] for key in ("rowptr", "truth_idx", "idf32", "sums32", "q_rowptr",
                                                                     "q_cols", "q_maxint")})
    return path


def _sweep_floor(shared, geometry, problem, sparse_tiles, status):
    """The `sparse_tiles` floors of test_gpu_guards.py; for the wide descending epochs also more than an epoch's worth of
    sparse tiles for every query that must sweep more than one epoch (jaccard_cases.multi_epoch_queries) and was answered by
    the fast kernel (a query handed over reports no tiles)."""
    case = shared.case(problem, geometry)
    if problem == "second_posting_problem":
        assert sparse_tiles > 48
        return
    assert sparse_tiles > 72
    if geometry == "wide":
        multi = jc.multi_epoch_queries(case, geometry, shared.expected((problem, geometry), case))
        answered = int(np.sum(multi & (np.asarray(status) == 0)))
        print("wide descending epochs: queries that sweep more than one epoch", int(multi.sum()), "answered fast", answered)
        assert answered >= 1 and sparse_tiles > jc.GEOMETRY[geometry]["epoch_tiles"] * answered


@pytest.mark.parametrize("problem", ["second_posting_problem", "descending_epochs_problem"])
@pytest.mark.parametrize("geometry", jc.GEOMETRIES)
def test_sweeps_on_the_product_build(shared, geometry, problem):
    """second posting: 4 tiles, most candidates receive two or three postings inside one sparse tile.  descending epochs: 13
    narrow / 35 wide tiles (two whole epochs of 16 and three tiles: sweeps cross epoch boundaries upwards and downwards, an
    entry's tile travels in its own byte over more than one epoch, 3-tile pointer blocks meet 16-tile epochs in both corners
    of `block_start`).  Wall time of the wide descending case (1,003,520 rows, 11.4M postings, 72 queries), the largest here,
    measured next to an MI355X on 16 CPU threads: generation 1.5 s, oracle 0.01 s, index build 0.2 s, both entries on the
    device 0.007 s (on an 8-thread machine without a GPU: generation 4.0 s, oracle 0.6 s); the bounds-checking child takes the
    arrays and the expected rows from a file and adds 0.7 s.  Counters observed: narrow second posting sparse_tiles 288,
    sparse_redos 48; wide 144 / 0; narrow descending epochs sparse_tiles 860, dense_tiles 84, sparse_redos 2; wide 2,830 / 72
    / 35, with 67 of the 72 queries bound to sweep more than one epoch (floor 16 * 67 = 1,072)."""
    case = shared.case(problem, geometry)
    index = shared.index(problem, geometry)
    assert index.info()["tiles"] == case["tiles"]
    stats, status = _both_entries(index, case, shared.expected((problem, geometry), case))
    print(geometry, problem, _ledger(stats))
    if problem == "second_posting_problem":
        assert stats["dense_queries"] == 0
    _sweep_floor(shared, geometry, problem, stats["sparse_tiles"], status)


@pytest.mark.parametrize("problem", ["second_posting_problem", "descending_epochs_problem"])
@pytest.mark.parametrize("geometry", jc.GEOMETRIES)
def test_sweeps_under_the_bounds_checking_build(shared, tmp_path_factory, geometry, problem):
    """The same problems through a -DDS_BOUNDS_CHECK build in a fresh process: no data-dependent global index (row records,
    list pointers, posting quads, forward index, output) leaves its array in either geometry."""
    case = shared.case(problem, geometry)
    expected = shared.expected((problem, geometry), case)
    outcome = _under_the_bounds_checking_build(problem, geometry, _saved(tmp_path_factory, problem, case, expected))
    summary = {key: value for key, value in outcome.items() if key != "status"}
    print(geometry, problem, summary)
    assert outcome["tiles"] == case["tiles"], summary
    assert outcome["bounds_record"] == [0, 0, 0], summary
    assert outcome["equal"] and outcome["device_equal"] and outcome["descending"] and outcome["error_queries"] == 0, summary
    if problem == "second_posting_problem":
        assert outcome["dense_queries"] == 0, summary
    _sweep_floor(shared, geometry, problem, outcome["sparse_tiles"], outcome["status"])


@pytest.mark.parametrize("tied", [False, True])
@pytest.mark.parametrize("geometry", jc.GEOMETRIES)
def test_epoch_redo(shared, geometry, tied):
    """candidates + 230 rows above the cut in the SECOND tile of an epoch of epoch_tiles sparse tiles (rows in the caller's
    order, DS_SORT_ROWS=0): the tile overflows the buffer, the whole epoch is processed again under a tightened cut and an
    admission floor.  distinct: it then fits -- at most 3 redos (the floor admits (trigger - 64) >> (retry - 1) rows: the third
    repetition asks for a quarter of the buffer), far from the give-up bound `++sparse_retries > 5`.  tied: no cut separates
    the rows; the query ends on the literal kernel as overflow_sparse (after exactly 5 counted redos) or as ties (the
    admission floor reached the k best: fewer redos) -- the counters cannot say which comes first, their sum is pinned and
    the split printed (observed in both geometries: distinct 1 redo, tied ties 1 after 1 redo)."""
    case = shared.case("redo_problem", geometry, tied)
    index = shared.index("redo_problem", geometry, tied, sort_rows=False)
    assert index.info()["tiles"] == jc.GEOMETRY[geometry]["epoch_tiles"] + 2
    stats, status = _both_entries(index, case, shared.expected(("redo_problem", geometry, tied), case))
    print(geometry, "redo", "tied" if tied else "distinct", _ledger(stats))
    reasons = stats["dense_reasons"]
    if tied:
        assert stats["sparse_redos"] >= 1 and stats["dense_queries"] == 1 and status[0] == 1
        assert reasons["overflow_sparse"] + reasons["ties"] == 1 and sum(reasons.values()) == 1
        if reasons["overflow_sparse"] == 1:
            assert stats["sparse_redos"] == 5
        else:
            assert stats["sparse_redos"] <= 5
    else:
        assert 1 <= stats["sparse_redos"] <= 3 and stats["dense_queries"] == 0 and status[0] == 0
        assert stats["sparse_tiles"] >= jc.GEOMETRY[geometry]["epoch_tiles"] + 2      # the epoch, and its first two tiles again
    # with the rows in sums32 order (the default) the answers are the same, whatever path serves them
    sorted_index = shared.index("redo_problem", geometry, tied)
    assert np.array_equal(sorted_index.top_k(case["q_rowptr"], case["q_cols"], case["q_maxint"], case["k"]),
                          shared.expected(("redo_problem", geometry, tied), case))


# ---- the hand-over ledger ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", jc.FEW_K)
@pytest.mark.parametrize("geometry", jc.GEOMETRIES)
def test_few_is_handed_over_at_k_minus_one_positive_rows_only(shared, geometry, k):
    """Reason 5: `m < k` after the last tile.  Three queries whose only column is held by k-1, k and k+1 rows (alternating
    between two tiles of the internal order): nothing is pruned before k candidates exist, so m is the number of positive
    rows -- `<=` in place of `<` hands the second query over as well, a miscounted tile loses a row and hands over the
    second or third.  (At k rows the final cut comes from a selection over exactly k keys.)"""
    whole = shared.case("few_problem", geometry)
    case = jc.select_queries(whole, whole["queries_of_k"][k], k)
    stats, status = _both_entries(shared.index("few_problem", geometry), case, shared.expected(("few_problem", geometry, k), case))
    print(geometry, "few", "k", k, _ledger(stats), "status", status.tolist())
    assert status.tolist() == [1, 0, 0]
    assert stats["dense_reasons"] == dict(zip(REASONS, (0, 0, 0, 0, 0, 1)))
    assert stats["exact_candidates"] >= 2 * k          # the two fast queries evaluate their k (k + 1) rows exactly


@pytest.mark.parametrize("geometry", jc.GEOMETRIES)
def test_shape_counts_exactly_the_queries_its_conditions_name(shared, geometry):
    """Reason 0 at the head of the kernel: `n > 128 || !(maxint > 0) || !(maxint < 1e30)` and, once the idf mass is known,
    `maxint32 < mass * 0.999f`.  Queries that differ only in max_intersection_possible: the exact total and total * 0.9995
    stay fast, total * 0.99, 0, -1, 1e30 and inf go; 128 columns stay, 129 go.  The NaN query is the reference's own error
    (no row compares >= a NaN threshold: "top_matches.shape[0] != self.top_n"), so it is run alone and both sides must raise;
    its reason is read from ds_jaccard_sync's statistics, which are filled before the error is returned."""
    import doppel_speller_amd as ds
    whole = shared.case("shape_problem", geometry)
    index = shared.index("shape_problem", geometry)
    nan_query = int(np.nonzero(np.isnan(whole["q_maxint"]))[0][0])
    others = [q for q in range(whole["q_maxint"].shape[0]) if q != nan_query]
    case = jc.select_queries(whole, others, whole["k"])
    stats, status = _both_entries(index, case, shared.expected(("shape_problem", geometry), case))
    print(geometry, "shape", _ledger(stats), "status", status.tolist())
    assert status.tolist() == whole["handed_over"][others].astype(int).tolist()
    assert stats["dense_reasons"] == dict(zip(REASONS, (6, 0, 0, 0, 0, 0)))
    alone = jc.select_queries(whole, [nan_query], whole["k"])
    with pytest.raises(Exception, match="top_matches.shape"):
        shared.oracle.jaccard_topk(*jc.arrays(alone))
    with pytest.raises(Exception, match="top_matches.shape"):
        index.top_k(alone["q_rowptr"], alone["q_cols"], alone["q_maxint"], alone["k"])
    raw = (ctypes.c_int64 * 32)()
    assert ds._lib.lib().ds_jaccard_sync(index.handle, ds._lib.pointer(None), raw) == -3      # DS_E_TOP_N
    assert list(raw)[16:22] == [1, 0, 0, 0, 0, 0] and raw[0] == 1


@pytest.mark.parametrize("tied", [False, True])
@pytest.mark.parametrize("geometry", jc.GEOMETRIES)
def test_overflow_inside_a_dense_tile(shared, geometry, tied):
    """candidates + 230 non-twin rows above the first cut inside ONE densely scanned tile (tile 1 of 3, rows in the caller's
    order; two columns held by every row keep the essential quads per tile above sparse_quads until the cut has risen).
    distinct: the scan overflows, the cut is tightened from the buffered sample, the same rows are scanned again and fit:
    nothing is handed over, and tiles 0 AND 1 are counted dense (tile 2, under the risen cut, may be sparse).  There is no
    counter of the dense retries themselves: that the overflow happened is the CPU test's statement about the input.
    tied: the retry meets the same rows; the query ends as overflow_dense (`++retries > 6`) or, when the admission floor
    reaches the tied value first, as ties -- the counters cannot say which, the sum is pinned and the split printed (observed
    in both geometries: ties 1, overflow_dense 0; distinct: dense_tiles 2, sparse_tiles 1, selections 5).  The other site of
    reason 3, "nothing to tighten with" (`force_select` with m < k), cannot be reached at all: a forced selection follows
    the bootstrap (m = 1 or 2 samples per thread >= k by the k classes) or an overflow (m = kCandidates > 512 >= k)."""
    case = shared.case("overflow_dense_problem", geometry, tied)
    index = shared.index("overflow_dense_problem", geometry, tied, sort_rows=False)
    stats, status = _both_entries(index, case, shared.expected(("overflow_dense_problem", geometry, tied), case))
    print(geometry, "overflow_dense", "tied" if tied else "distinct", _ledger(stats))
    reasons = stats["dense_reasons"]
    if tied:
        assert reasons["overflow_dense"] + reasons["ties"] >= 1 and sum(reasons.values()) == 1
        assert status[0] == 1 and stats["sparse_redos"] == 0
    else:
        assert stats["dense_queries"] == 0 and status[0] == 0
        assert stats["dense_tiles"] >= 2 and stats["dense_tiles"] + stats["sparse_tiles"] == 3 and stats["sparse_redos"] == 0
        assert stats["selections"] >= 3          # the bootstrap, tile 0's rows, the overflow's tightening
    sorted_index = shared.index("overflow_dense_problem", geometry, tied)
    assert np.array_equal(sorted_index.top_k(case["q_rowptr"], case["q_cols"], case["q_maxint"], case["k"]),
                          shared.expected(("overflow_dense_problem", geometry, tied), case))
