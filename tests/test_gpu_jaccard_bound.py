"""The skip-set bound at the band's edge and the 16 membership bits per posting of the Jaccard top-k kernel, in both
geometries: the cases of jaccard_bound_cases.py (proved in test_jaccard_bound_cases_cpu.py), every one compared with
oracle.jaccard_topk bit for bit through the host and the device entry with DS_GEOMETRY forced, and once through a
-DDS_BOUNDS_CHECK build in a fresh process.  The witness of the bound is `skipped_columns` of ds_jaccard_sync: with one query
per launch it is the number of columns the query's LAST selection skipped."""
import time

import numpy as np
import pytest

import jaccard_bound_cases as bc
import jaccard_cases as jc
from test_gpu_guards import _under_the_bounds_checking_build
from test_gpu_jaccard_geometries import REASONS, _both_entries, _ledger, _saved

pytestmark = pytest.mark.gpu


class _Shared:
    """Cases and their indexes (built under DS_GEOMETRY), each made once per module."""

    def __init__(self, oracle):
        self.oracle, self.cases, self.indexes = oracle, {}, {}

    def case(self, name, *args):
        if (name,) + args not in self.cases:
            begin = time.perf_counter()
            self.cases[(name,) + args] = getattr(bc, name)(*args)
            print("[wall] generation", name, args, "%.2f s" % (time.perf_counter() - begin))
        return self.cases[(name,) + args]

    def index(self, geometry, name, *args):
        import doppel_speller_amd as ds
        if (geometry, name) + args not in self.indexes:
            case = self.case(name, *args)
            with pytest.MonkeyPatch.context() as patch:       # the environment is read by ds_index_create only
                patch.setenv("DS_GEOMETRY", geometry)
                self.indexes[(geometry, name) + args] = ds.TruthIndex(case["rowptr"], case["truth_idx"], case["idf32"],
                                                                      case["sums32"])
        index = self.indexes[(geometry, name) + args]
        assert index.info()["tile_rows"] == jc.GEOMETRY[geometry]["tile_rows"]
        return index

    def run(self, index, case):
        expected = self.oracle.jaccard_topk(*jc.arrays(case))
        stats, status = _both_entries(index, case, expected)
        print(_ledger(stats), "status", status.tolist())
        return stats, status, expected


@pytest.fixture(scope="module")
def shared(oracle):
    return _Shared(oracle)


def _checked_build(tmp_path_factory, geometry, name, case, expected):
    outcome = _under_the_bounds_checking_build(name, geometry, _saved(tmp_path_factory, name, case, expected))
    summary = {key: value for key, value in outcome.items() if key != "status"}
    print(geometry, name, summary)
    assert outcome["bounds_record"] == [0, 0, 0], summary
    assert outcome["equal"] and outcome["device_equal"] and outcome["error_queries"] == 0, summary
    return outcome


@pytest.mark.parametrize("k", bc.DECISIVE_K)
@pytest.mark.parametrize("geometry", jc.GEOMETRIES)
def test_decisive_column_is_skipped(shared, geometry, k):
    """One column's prefix mass lies between the bound from the index's smallest sums32 and the bound from the band's edge,
    5 % of maxint from either, under every cut the query can hold: three columns are skipped, not two.  The rows that
    depend on it: rows of skipped columns only, the best rows of the index (completed from the signature with the newly
    skipped column), rows below the band's edge in a tile the sweep visits."""
    case = dict(shared.case("decisive_problem", geometry), k=k)
    stats, status, _ = shared.run(shared.index(geometry, "decisive_problem", geometry), case)
    assert status.tolist() == [0] and stats["dense_queries"] == 0
    assert stats["sparse_tiles"] >= 2                       # tiles 0 and 1 lie inside the band, below the start tile
    expected_count = bc.skipped_count(case, 0, bc.kth_value(case, 0, k)[0])
    assert expected_count == 3 and stats["skipped_columns"] == expected_count


@pytest.mark.parametrize("geometry", jc.GEOMETRIES)
def test_membership_bits_8_to_15_decide(shared, geometry):
    """Sixteen skipped columns own the signature bits 0..15; rows that hold the columns of bits 8..15 (or 0..7) on top of the
    one essential column are the answer, rows without them -- the same sums32 -- lie below every cut."""
    case = shared.case("high_bits_problem", geometry)
    stats, status, expected = shared.run(shared.index(geometry, "high_bits_problem", geometry), case)
    assert status.tolist() == [0] and stats["skipped_columns"] == 16 and stats["sparse_tiles"] >= 2
    assert np.isin(expected[0], case["high"]).sum() >= 3 and np.isin(expected[0], case["low"]).sum() >= 3
    assert not np.isin(expected[0], case["without"]).any()


@pytest.mark.parametrize("geometry", jc.GEOMETRIES)
def test_skipped_columns_above_half_of_the_mass(shared, geometry):
    """Round 4's first 16-bit tables capped their entries and were wrong whenever the skipped columns held more than half of
    the query's mass: three columns, 24,581 rows, k = 1.  Narrow: the answer lies in a sparsely swept tile ABOVE the start
    tile and passes the sweep only if its membership bits are credited with the whole 6.2 of 10 that the two skipped columns
    hold (proved on the CPU: with an entry capped at 32,000 units it stays 0.07 * maxint below the gate)."""
    case = shared.case("capped_table_problem")
    stats, status, expected = shared.run(shared.index(geometry, "capped_table_problem"), case)
    assert expected.tolist() == [case["winner"].tolist()] and status.tolist() == [0]
    if geometry == "narrow":
        assert stats["skipped_columns"] == 2                 # the start tile ended in a selection: A and B are skipped
        assert stats["dense_tiles"] == 1 and stats["sparse_tiles"] >= 1       # tile 2, sparsely


@pytest.mark.parametrize("n", range(len(bc.PADDING_LISTS)))
@pytest.mark.parametrize("geometry", jc.GEOMETRIES)
def test_padding_next_to_rows_that_qualify(shared, geometry, n):
    """Essential lists of 1, 2, 3 and 5 postings per tile, one of them also in the last tile of a single row: the answer is
    exactly the lists' rows, and nothing a padding entry or an idle lane takes from the word behind the tile gets through
    (an entry that did would leave the tile: `bounds_record`, and `error_queries`, stay clean in the checked build below)."""
    whole = shared.case("padding_problem", geometry)
    case = jc.select_queries(whole, [n], whole["k_of_query"][n])
    stats, status, expected = shared.run(shared.index(geometry, "padding_problem", geometry), case)
    assert np.array_equal(np.sort(expected[0]), whole["p%d" % bc.PADDING_LISTS[n]]) and status.tolist() == [0]
    assert stats["sparse_tiles"] >= 2


@pytest.mark.parametrize("geometry", jc.GEOMETRIES)
def test_no_threshold_falls_back(shared, geometry):
    """Six and nine positive rows for k = 10: the cut stays 0, the bound stays FLT_MIN (no division, no band edge), nothing
    is skipped, and both queries end on the literal kernel as "few"."""
    whole = shared.case("padding_problem", geometry)
    case = jc.select_queries(whole, [4, 5], 10)
    stats, status, _ = shared.run(shared.index(geometry, "padding_problem", geometry), case)
    assert status.tolist() == [1, 1] and stats["dense_reasons"] == dict(zip(REASONS, (0, 0, 0, 0, 0, 2)))
    assert stats["skipped_columns"] == 0


@pytest.mark.parametrize("name", ["decisive_problem", "high_bits_problem", "capped_table_problem", "padding_problem",
                                  "no_threshold"])
@pytest.mark.parametrize("geometry", jc.GEOMETRIES)
def test_under_the_bounds_checking_build(shared, tmp_path_factory, geometry, name):
    """Every case once through the -DDS_BOUNDS_CHECK build: no data-dependent global index leaves its array (a padding entry
    that passed the collect sweep would: its row lies behind the tile).  no_threshold: queries 4 and 5 of padding_problem at
    k = 10, which the fast kernel sweeps to the end without a cut before it hands them over."""
    if name == "capped_table_problem":
        case = shared.case(name)
    elif name == "padding_problem":
        whole = shared.case(name, geometry)
        case = jc.select_queries(whole, [3], whole["k_of_query"][3])
    elif name == "no_threshold":
        case = jc.select_queries(shared.case("padding_problem", geometry), [4, 5], 10)
    else:
        case = shared.case(name, geometry)
    expected = shared.oracle.jaccard_topk(*jc.arrays(case))
    outcome = _checked_build(tmp_path_factory, geometry, name, case, expected)
    if name == "no_threshold":
        assert outcome["dense_queries"] == 2 and outcome["status"] == [1, 1]
        return
    least = {("capped_table_problem", "wide"): 0, ("capped_table_problem", "narrow"): 1}.get((name, geometry), 2)
    assert outcome["dense_queries"] == 0 and outcome["sparse_tiles"] >= least
