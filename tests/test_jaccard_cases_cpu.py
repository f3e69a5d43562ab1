"""jaccard_cases.py proved from its inputs alone, without a GPU: the geometry table equals the kernels' #defines, and every
case has the tiles, the rows above the cut, the ties, the positive rows and the pointer-block spans it was built for.  What
the GPU tests (test_gpu_jaccard_geometries.py, test_gpu_guards.py) then observe on the device is a statement about the
kernel, not about an input that drifted."""
import functools
import glob
import os
import re

import numpy as np
import pytest

import jaccard_cases as jc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "doppel-speller_amd", "csrc")
MOVE_THE_TABLE = ("tests/jaccard_cases.py GEOMETRY no longer equals the kernel's constants: move the table (and read what the "
                  "cases built on it still reach) in the same change")

second_posting = functools.lru_cache(maxsize=None)(jc.second_posting_problem)
descending_epochs = functools.lru_cache(maxsize=None)(jc.descending_epochs_problem)
redo = functools.lru_cache(maxsize=None)(jc.redo_problem)
overflow_dense = functools.lru_cache(maxsize=None)(jc.overflow_dense_problem)
few = functools.lru_cache(maxsize=None)(jc.few_problem)
shape = functools.lru_cache(maxsize=None)(jc.shape_problem)


def _define(text, name):
    found = re.search(r"^#define\s+%s\s+(\d+)\b" % name, text, re.M)
    assert found, name
    return int(found.group(1))


@pytest.mark.parametrize("geometry", jc.GEOMETRIES)
def test_geometry_table_equals_the_kernels_defines(geometry):
    with open(os.path.join(CSRC, "ds_jaccard_%s.hip" % geometry)) as handle:
        text = handle.read()
    table = jc.GEOMETRY[geometry]
    for key, name in (("threads", "DS_THREADS"), ("candidates", "DS_CANDIDATES"), ("ptr_tiles", "DS_PTR_TILES"),
                      ("epoch_tiles", "DS_EPOCH_TILES")):
        assert table[key] == _define(text, name), (geometry, name, MOVE_THE_TABLE)
    constant = {"narrow": "kNarrowTileRows", "wide": "kWideTileRows"}[geometry]
    assert re.search(r"^#define\s+DS_TILE_ROWS\s+ds::%s\b" % constant, text, re.M), (geometry, MOVE_THE_TABLE)
    values = set()
    for path in glob.glob(os.path.join(CSRC, "*")):
        with open(path, errors="replace") as handle:
            values.update(int(v) for v in re.findall(r"\b%s\s*=\s*(\d+)" % constant, handle.read()))
    assert values == {table["tile_rows"]}, (geometry, constant, values, MOVE_THE_TABLE)


def test_constants_the_table_does_not_hold():
    with open(os.path.join(CSRC, "ds_jaccard_impl.inc")) as handle:
        text = handle.read()
    assert int(re.search(r"kSelectSlack\s*=\s*(\d+)", text).group(1)) == jc.SELECT_SLACK, MOVE_THE_TABLE
    assert int(re.search(r"kMaxSelectK\s*=\s*(\d+)", text).group(1)) == jc.MAX_SELECT_K, MOVE_THE_TABLE
    assert int(re.search(r"args\.sparse_quads\s*=\s*(\d+)", text).group(1)) == jc.SPARSE_QUADS, MOVE_THE_TABLE
    assert re.search(r"kProbeMaxK\s*=\s*kThreads\s*/\s*4\b", text), MOVE_THE_TABLE
    assert re.search(r"second_sample\s*=\s*k > kProbeMaxK && k <= 2 \* kProbeMaxK", text), MOVE_THE_TABLE
    assert re.search(r"kSelectTrigger\s*=\s*kCandidates - kSelectSlack", text), MOVE_THE_TABLE
    assert re.search(r"\+\+sparse_retries > 5\b", text), "the redo bound of test_gpu_jaccard_geometries.py"
    with open(os.path.join(CSRC, "ds_common.h")) as handle:
        assert int(re.search(r"kMaxQueryColumns\s*=\s*(\d+)", handle.read()).group(1)) == jc.MAX_QUERY_COLUMNS


def test_derived_k_classes():
    assert jc.probe_max_k("narrow") == 64 and jc.probe_max_k("wide") == 128
    assert jc.k_class_edges("narrow") == (64, 65, 128, 129, 512) and jc.k_class_edges("wide") == (128, 129, 256, 257, 512)
    assert jc.select_trigger("narrow") == 640 and jc.select_trigger("wide") == 1344
    for geometry in jc.GEOMETRIES:
        classes = jc.k_classes(geometry)
        p, edges = jc.probe_max_k(geometry), jc.k_class_edges(geometry)
        assert classes["first_sample"] == (1, p) and classes["second_sample"] == (p + 1, 2 * p)
        assert classes["flood"] == (2 * p + 1, 512)
        # every class has a k on each of its edges; 2 * threads samples fit below the selection trigger
        assert {edges[0]} <= set(range(*classes["first_sample"])) | {classes["first_sample"][1]}
        assert edges[1] == classes["second_sample"][0] and edges[2] == classes["second_sample"][1]
        assert edges[3] == classes["flood"][0] and edges[4] == classes["flood"][1]
        assert 2 * jc.GEOMETRY[geometry]["threads"] <= jc.select_trigger(geometry)


@pytest.mark.parametrize("geometry", jc.GEOMETRIES)
def test_tile_counts(geometry):
    g = jc.GEOMETRY[geometry]
    assert jc.tiles_of(jc.tie_problem(geometry), geometry) == 3
    assert jc.tiles_of(jc.ragged_problem(geometry), geometry) == 4       # 3 tiles plus one row
    for case, tiles in ((second_posting(geometry), 4), (redo(geometry, False), g["epoch_tiles"] + 2),
                        (redo(geometry, True), g["epoch_tiles"] + 2), (few(geometry), 3), (shape(geometry), 3),
                        (overflow_dense(geometry, False), 3), (overflow_dense(geometry, True), 3),
                        (descending_epochs(geometry), {"narrow": 13, "wide": 35}[geometry])):
        assert jc.tiles_of(case, geometry) == tiles == case["tiles"]
    assert second_posting("wide")["sums32"].shape[0] == 114688 and descending_epochs("wide")["sums32"].shape[0] == 1003520
    assert redo("wide", True)["strong_rows"].shape[0] == 1702 and redo("narrow", True)["strong_rows"].shape[0] == 998


def test_the_tie_problem_has_its_twins():
    case = jc.tie_problem("narrow")
    columns = jc.columns_of_rows(case, np.arange(6001))
    assert len({columns[row] for row in range(6000)}) == 1 and columns[6000] != columns[0]
    assert np.unique(case["sums32"][:6000]).shape[0] == 1
    assert all(tuple(jc.query_columns(case, q).tolist()) == columns[0] for q in range(0, 40, 4))


@pytest.mark.parametrize("geometry", jc.GEOMETRIES)
def test_second_posting_rows_hold_several_of_a_querys_rare_columns(geometry):
    case = second_posting(geometry)
    rare_of = {row: [c for c in columns if 6 <= c < 18] for row, columns in jc.columns_of_rows(case, case["cluster_rows"]).items()}
    assert all(len(rare) >= 3 for rare in rare_of.values())
    tile_rows = jc.GEOMETRY[geometry]["tile_rows"]
    assert set((case["cluster_rows"] // tile_rows).tolist()) == {0, 1, 2, 3}
    for q in range(48):
        mine = set(jc.query_columns(case, q).tolist())
        assert len(mine) == 10 and set(range(6)) <= mine
        twice = sum(len(mine.intersection(rare)) >= 2 for rare in rare_of.values())
        assert twice > 0.2 * len(rare_of), (q, twice)          # hundreds of rows with two or more postings of the query's rare columns
    assert jc.quads_upper_bound(case, 0, geometry) > jc.SPARSE_QUADS * 4      # the dense columns must be skipped for a sparse tile ...
    dense_free = dict(case, q_rowptr=np.array([0, 4]), q_cols=jc.query_columns(case, 0)[6:])
    assert jc.quads_upper_bound(dense_free, 0, geometry) <= jc.SPARSE_QUADS * 4     # ... and then it is one


def _kth_best_before(case, jaccard, tile, tile_rows):
    before = np.sort(jaccard[:tile * tile_rows])[::-1]
    assert before[case["k"] - 1] > 0.0                      # the tiles swept before hold k positive rows: a cut exists
    return before[case["k"] - 1]


@pytest.mark.parametrize("tied", [False, True])
@pytest.mark.parametrize("problem", ["redo", "overflow_dense"])
@pytest.mark.parametrize("geometry", jc.GEOMETRIES)
def test_more_rows_above_the_cut_in_one_tile_than_the_buffer_holds(geometry, problem, tied):
    """Rows in the caller's order (both cases run under DS_SORT_ROWS=0): tile = row // tile_rows, swept from tile 0 up."""
    g = jc.GEOMETRY[geometry]
    case = {"redo": redo, "overflow_dense": overflow_dense}[problem](geometry, tied)
    tile_rows, tile = g["tile_rows"], case["overflowing_tile"]
    _, jaccard = jc.jaccard_rows(case, 0)
    cut = _kth_best_before(case, jaccard, tile, tile_rows)
    inside = np.arange(tile * tile_rows, (tile + 1) * tile_rows)
    above = inside[jaccard[inside] > cut]
    assert above.shape[0] == g["candidates"] + 230 > g["candidates"] and np.array_equal(above, case["strong_rows"])
    assert (case["strong_rows"] // tile_rows == tile).all() and (case["weak_rows"] // tile_rows == 0).all()
    # no other tile comes near the buffer's size
    for other in range(case["tiles"]):
        if other != tile:
            rows = np.arange(other * tile_rows, (other + 1) * tile_rows)
            assert np.sum(jaccard[rows] >= jaccard[case["weak_rows"]].min()) <= 300
    values = np.sort(jaccard[case["strong_rows"]])
    if tied:      # within the reference's 1e-6 of each other (here: equal): no threshold separates them
        assert values[-1] - values[0] <= 1e-6 and np.unique(case["sums32"][case["strong_rows"]]).shape[0] == 1
    else:         # no two within 1e-6: a cut between any two neighbours exists
        assert np.diff(values).min() > 1e-6
    columns = jc.columns_of_rows(case, case["strong_rows"])
    assert len(set(columns.values())) == case["strong_rows"].shape[0]          # no two are twins
    # sparse or dense, as the case claims, under the cut that tile 0 leaves behind
    idf = case["idf32"][jc.query_columns(case, 0)].astype(np.float64)
    pre = cut / (1.0 + cut) * (float(case["sums32"].min()) + float(case["q_maxint"][0]))
    if problem == "redo":
        assert jc.quads_upper_bound(case, 0, geometry) <= jc.SPARSE_QUADS * case["tiles"]
        assert case["overflowing_tile"] == 2 and case["tiles"] == g["epoch_tiles"] + 2    # second tile of the epoch 1..epoch_tiles
    else:
        # D1 and D2 (held by every row) cannot be skipped: already the smaller of them outweighs `pre`; in both geometries
        # they alone are more quads per tile than sparse_quads
        everyone = np.diff(case["rowptr"])[jc.query_columns(case, 0)] == case["sums32"].shape[0]
        assert everyone.sum() == 2 and idf[everyone].min() > 1.5 * pre
        assert 2 * (tile_rows // 4) > jc.SPARSE_QUADS
        assert (jaccard[np.setdiff1d(np.arange(case["sums32"].shape[0]), np.concatenate((case["strong_rows"], case["weak_rows"])))]
                < 0.1 * jaccard[case["weak_rows"]].min()).all()


@pytest.mark.parametrize("geometry", jc.GEOMETRIES)
def test_few_has_exactly_the_positive_rows_it_names(oracle, geometry):
    case = few(geometry)
    tile_rows = jc.GEOMETRY[geometry]["tile_rows"]
    n_rows = case["sums32"].shape[0]
    position = np.empty(n_rows, dtype=np.int64)
    position[jc.internal_order(case)] = np.arange(n_rows)
    assert case["few_sizes"] == [0, 1, 2, 9, 10, 11, 99, 100, 101]
    for k in jc.FEW_K:
        for q, positive in zip(case["queries_of_k"][k], (k - 1, k, k + 1)):
            assert jc.query_columns(case, q).shape[0] == 1
            scores, jaccard = jc.jaccard_rows(case, q)
            assert np.sum(scores > 0) == np.sum(jaccard > 0) == positive == case["few_sizes"][q]
            if positive >= 2:     # spread over the tiles of the index as the device stores it
                assert np.unique(position[scores > 0] // tile_rows).shape[0] >= 2
        selected = jc.select_queries(case, case["queries_of_k"][k], k)
        expected = oracle.jaccard_topk(*jc.arrays(selected))
        assert np.array_equal(expected[0], np.arange(n_rows - 1, n_rows - 1 - k, -1))   # fewer than k positive: the k largest indexes
        for row in (1, 2):
            assert (jc.jaccard_rows(selected, row)[1][expected[row]] > 0).all()
    columns = jc.columns_of_rows(case, np.arange(n_rows))
    assert len(set(columns.values())) == n_rows                                          # no twins


@pytest.mark.parametrize("geometry", jc.GEOMETRIES)
def test_shape_names_the_queries_the_conditions_send_away(geometry):
    """The conditions at the head of the fast kernel, restated: n > 128, not (maxint > 0), not (maxint < 1e30),
    float32(maxint) < mass * 0.999f with mass = the float64 total of the columns' float32 idf * (1 + 2^-18), rounded up."""
    case = shape(geometry)
    handed_over = []
    with np.errstate(invalid="ignore"):
        for q in range(case["q_maxint"].shape[0]):
            columns, maxint = jc.query_columns(case, q), case["q_maxint"][q]
            mass = np.float32(case["idf32"][columns].astype(np.float64).sum() * (1.0 + 3.814697265625e-06))
            mass = np.nextafter(mass, np.float32(np.inf))
            handed_over.append(bool(columns.shape[0] > jc.MAX_QUERY_COLUMNS or not maxint > 0.0 or not maxint < 1e30
                                    or np.float32(maxint) < mass * np.float32(0.999)))
    assert handed_over == case["handed_over"].tolist() and sum(handed_over) == 7
    assert np.diff(case["q_rowptr"]).tolist() == [12] * 8 + [128, 129]
    for q in range(1, 8):
        assert np.array_equal(jc.query_columns(case, q), jc.query_columns(case, 0))
    total = case["q_maxint"][0]
    assert total == sum(float(np.log(case["sums32"].shape[0] / np.diff(case["rowptr"])[c])) for c in jc.query_columns(case, 0))
    assert case["q_maxint"][1] == total * 0.9995 and case["q_maxint"][2] == total * 0.99
    assert case["q_maxint"][3:7].tolist() == [0.0, -1.0, 1e30, np.inf] and np.isnan(case["q_maxint"][7])


@pytest.mark.parametrize("geometry", jc.GEOMETRIES)
def test_descending_epochs_span_relations(oracle, geometry):
    g = jc.GEOMETRY[geometry]
    case = descending_epochs(geometry)
    n_tiles, ranges = case["tiles"], jc.tile_ranges(case, geometry)
    assert n_tiles > 2 * g["epoch_tiles"] and case["k"] == 100
    spans = np.array([jc.pointer_span(geometry, jc.query_columns(case, q).shape[0], n_tiles) for q in range(72)])
    starts = np.array([jc.start_tile(case, q, ranges) for q in range(72)])
    one, two, three = (np.array(case["families"][name]) for name in ("one", "two", "three"))
    # one: from the last tile down, with a pointer block of at least ptr_tiles but shorter than an epoch
    assert (starts[one] == n_tiles - 1).all()
    assert (spans[one] >= g["ptr_tiles"]).all() and (spans[one] < g["epoch_tiles"]).all()
    # two: a block of an epoch or more, shorter than every block of family three
    assert (spans[two] >= g["epoch_tiles"]).all() and spans[two].max() < spans[three].min()
    # three: starts within an epoch of tile 0, and its block is longer than the tiles below the start (the block of a
    # descending epoch would begin in front of tile 0: block_start = max(0, ...))
    assert (starts[three] < g["epoch_tiles"]).all() and (starts[three] > 0).all() and (spans[three] > starts[three]).all()
    expected = oracle.jaccard_topk(*jc.arrays(case))
    multi = jc.multi_epoch_queries(case, geometry, expected)
    if geometry == "wide":   # the floor of the device test: more than 16 sparse tiles for each of these
        assert multi[one].sum() >= 12 and multi[two].sum() >= 12 and multi[three].sum() >= 12, multi.reshape(3, 24).sum(axis=1)
