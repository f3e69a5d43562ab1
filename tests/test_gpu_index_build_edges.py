"""The device index build at its edge shapes, three ways: the host's image (ds_index_create), the device's
(ds_index_create_device) and the NumPy restatement of the rule (index_build_cases.expected_image, pinned against the host
at three tile sizes by test_index_build_edges_cpu.py) -- every array and scalar, byte for byte, no tolerance.  The inputs
are the named problems of index_build_cases (fewer rows than a wave, row, column and posting counts around every sort
pass, tile and scan boundary, no posting at all, NaNs and zeros of both signs in sums32, one row that raises literal_only,
hash groups whose largest row is a stray) and generated adversarial indexes (hypothesis)."""
import os

import numpy as np
import pytest

import index_build_cases as ic
from test_gpu_index_build import ARRAYS, SCALARS, _build, _same_image

pytestmark = pytest.mark.gpu
_SOAK = int(os.environ.get("DS_PROPERTY_EXAMPLES", "0"))


def _equals_expected(image, expected, what):
    for name in SCALARS:
        assert image[name] == expected[name], (what, name, image[name], expected[name])
    for name in ARRAYS:
        a, b = expected[name], image[name]
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.dtype, b.dtype, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            differ = np.nonzero(a.reshape(-1).view(np.uint8) != b.reshape(-1).view(np.uint8))[0]
            raise AssertionError((what, name, "bytes differ from the rule", differ.shape[0], "first at byte", int(differ[0]),
                                  a.reshape(-1)[differ[0] // a.itemsize], b.reshape(-1)[differ[0] // a.itemsize]))


def _three_way(problem, what, sort_rows=True, geometry=None):
    """Host and device images equal each other (and info()), and both equal the rule at the index's own tile size."""
    host = _build(problem, "host", geometry=geometry, sort_rows=sort_rows)
    device = _build(problem, "device", geometry=geometry, sort_rows=sort_rows)
    assert host.handle and device.handle, what                     # both creates succeeded
    image = _same_image(host, device)
    expected = ic.expected_image(*problem[:4], image["tile_rows"], sort_rows=sort_rows)
    _equals_expected(image, expected, what)
    host.close()
    return image, device


# ---- 1. the named problems -------------------------------------------------------------------------------------------
NAMED = ic.named_problems()
WIDE = {f"wide_tile_edges[{n}]": (lambda n=n: ic.tile_edges(n, ic.WIDE)) for n in ic.tile_edge_rows(ic.WIDE)}
WIDE["wide_nan_tiles"] = lambda: ic.nan_tiles(ic.WIDE)


@pytest.mark.parametrize("sort_rows", [True, False], ids=["sorted", "callers_order"])
@pytest.mark.parametrize("name", sorted(NAMED) + sorted(WIDE))
def test_named_problems_three_ways(name, sort_rows):
    wide = name in WIDE
    problem = (WIDE if wide else NAMED)[name]()
    image, device = _three_way(problem, name, sort_rows, "wide" if wide else "narrow")
    device.close()
    n = problem[5]
    tile_rows = ic.WIDE if wide else ic.NARROW
    assert image["tile_rows"] == tile_rows and image["n_tiles"] == (n + tile_rows - 1) // tile_rows
    assert image["rows_sorted"] == int(sort_rows) and image["row_cols_bytes"] == (4 if problem[4] > 65536 else 2)
    if name.startswith("no_postings"):
        assert image["n_quads"] == 0 and image["postings"].size == 0 and image["row_cols"].size == 0
    if name.startswith("one_bad_row") or "nan_tiles" in name:
        assert image["literal_only"] == 1
    if name.startswith(("rows_at", "columns_at", "postings_at", "tile_edges", "wide_tile_edges")) or name == "one":
        assert image["literal_only"] == 0
    if "nan_tiles" in name:     # what the tiles report: the NaN they start from (sorted); the first of the equal zeros
        assert image["n_tiles"] == (1 if name == "nan_tiles[64]" else 2)
        assert image["tile_sums_min"].view(np.uint32).tolist() == [0xffc00000 if sort_rows else 0x80000000, 0x7fc00000][:image["n_tiles"]]
        assert image["sums_min_bits"] == (0xffc00000 if sort_rows else 0x80000000)


@pytest.mark.parametrize("bad_row", [4999, 2500])
def test_one_row_raises_literal_only_and_its_repair_takes_it_back(bad_row):
    rowptr, truth_idx, idf32, sums32, v, n = ic.one_bad_row(bad_row)
    repaired = ic.true_sums(rowptr, truth_idx, idf32, n)
    for sums, flag in ((sums32, 1), (repaired, 0)):
        image, device = _three_way((rowptr, truth_idx, idf32, sums, v, n), ("one_bad_row", bad_row, flag))
        device.close()
        assert image["literal_only"] == flag


def test_ranks_saturate_in_an_index_without_postings():
    """65,537 rows without a column and with one sums32 value are one hash group: ranks 65,535, 65,535, 65,534 ... 1, 0."""
    image, device = _three_way(ic.no_postings(65537, values=(1.0,)), "no_postings[65537]")
    device.close()
    assert np.array_equal(image["records"][:, 5], np.minimum(np.arange(65536, -1, -1), 65535))


# ---- 2. generated indexes, and the index in use -----------------------------------------------------------------------
hypothesis = pytest.importorskip("hypothesis")
from hypothesis import HealthCheck, given, settings, strategies as st  # noqa: E402


def _top_k_equals_the_oracle(oracle, index, problem, queries, k):
    def answer(run):      # fewer than k rows may qualify (test_gpu_property.py): then both sides raise the reference's text
        try:
            return run()
        except Exception as error:  # noqa: BLE001 - the reference's own exception type
            return str(error)
    got = answer(lambda: index.top_k(*queries, k))
    expected = answer(lambda: oracle.jaccard_topk(*problem[:4], *queries, k))
    if isinstance(got, str) or isinstance(expected, str):
        assert isinstance(got, str) and isinstance(expected, str) and "top_matches.shape[0] != self.top_n" in got and \
            "top_matches.shape[0] != self.top_n" in expected, (got, expected)
        return
    assert index.sync()["error_queries"] == 0
    assert np.array_equal(got, expected)


@settings(max_examples=_SOAK or 60, deadline=None, suppress_health_check=list(HealthCheck), derandomize=not _SOAK)
@given(seed=st.integers(0, 2 ** 31 - 1),
       n_rows=st.one_of(st.integers(1, 300), st.integers(12200, 12400), st.integers(24500, 24700)),
       n_columns=st.integers(1, 400), shape=st.sampled_from(ic.SHAPES), sums=st.sampled_from(ic.SUMS), sort_rows=st.booleans())
def test_generated_indexes_three_ways_and_in_use(oracle, seed, n_rows, n_columns, shape, sums, sort_rows):
    problem = ic.adversarial_problem(seed, n_rows, n_columns, shape, sums)
    what = (seed, n_rows, n_columns, shape, sums, sort_rows)
    image, device = _three_way(problem, what, sort_rows)
    try:
        if sums == "true":      # the fields the image does not hold: stream, events, control block, forward widths
            assert image["literal_only"] == 0, what
            queries = ic.adversarial_queries(seed, n_rows, n_columns, shape)
            _top_k_equals_the_oracle(oracle, device, problem, queries, min(n_rows, 10))
    finally:
        device.close()


# ---- 3. truncated hashes ---------------------------------------------------------------------------------------------
def _truncated(problem, what):
    import doppel_speller_amd as ds
    option = ds._lib.lib().ds_index_build_option
    p_rowptr, p_idx, p_sums, _ = ic.internal_csr(problem[0], problem[1], problem[3])
    whole = ic.duplicate_ranks_rule(p_rowptr, p_idx, p_sums)
    differs = 0
    try:
        for hash_bits in ic.HASH_BITS + (64,):
            assert option(b"duplicate_hash_bits", hash_bits) == 0
            device = _build(problem, "device")
            ranks = device.image()["records"][:, 5]
            device.close()
            rule = ic.duplicate_ranks_rule(p_rowptr, p_idx, p_sums, hash_bits)
            assert np.array_equal(ranks, rule.astype(np.uint32)), (what, hash_bits)
            assert hash_bits != 64 or np.array_equal(rule, whole)
            differs += int(not np.array_equal(rule, whole))
    finally:
        assert option(b"duplicate_hash_bits", 0) == 0
    _three_way(problem, what)[1].close()      # back at 0: the host's ranks again
    return differs


@pytest.mark.parametrize("made_for", ic.HASH_BITS)
def test_truncated_hashes_with_a_stray_largest_row(made_for):
    assert _truncated(ic.stray_largest(made_for), ("stray_largest", made_for)) >= 1


@pytest.mark.parametrize("seed,n_rows,n_columns", [(1, 300, 40), (2, 12300, 9), (3, 2049, 400)])
def test_truncated_hashes_on_generated_twins(seed, n_rows, n_columns):
    _truncated(ic.adversarial_problem(seed, n_rows, n_columns, "twins", "few"), ("twins", seed, n_rows, n_columns))


# ---- 4. repetition ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nan_tiles", "few"])
@pytest.mark.parametrize("sort_rows", [True, False], ids=["sorted", "callers_order"])
def test_two_device_builds_give_the_same_bytes(name, sort_rows):
    problem = ic.nan_tiles(ic.NARROW) if name == "nan_tiles" else ic.adversarial_problem(9, 12345, 30, "single", "few")
    first, second = (_build(problem, "device", geometry="narrow", sort_rows=sort_rows) for _ in range(2))
    _same_image(first, second)
    first.close()
    second.close()
