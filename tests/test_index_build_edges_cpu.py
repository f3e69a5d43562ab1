"""The NumPy restatement of the whole index image (index_build_cases.expected_image) against the host build, and the
claims of the named edge problems, without a GPU.  ds_index_image_digest builds the host's image at ANY even tile size, so
the restatement is pinned on multi-tile images of a few rows (tile_rows 2 and 64) as well as on one-tile images (12288),
in the sorted internal order and in the caller's (DS_SORT_ROWS=0), before tests/test_gpu_index_build_edges.py holds both
builds against it.  Every claim of a problem's docstring that a GPU test relies on is asserted here from NumPy alone."""
import ctypes

import numpy as np
import pytest

import index_build_cases as ic

TILE_ROWS = (2, 64, 12288)
SMALL = ic.named_problems(max_rows=5000)
# two sizes for every shape x sums: 50 generated problems
SIZES = ((1, 1), (2, 3), (7, 400), (64, 17), (65, 2), (129, 40), (257, 131), (300, 90), (33, 9), (200, 300))
GENERATED = [(shape, sums, SIZES[(2 * i + j) % len(SIZES)] + (1000 + 10 * i + j,))
             for i, (shape, sums) in enumerate((a, b) for a in ic.SHAPES for b in ic.SUMS) for j in (0, 1)]


@pytest.fixture(scope="module")
def host_digest():
    from doppel_speller_amd import _lib
    library = ctypes.CDLL(_lib.build_library())

    def digest(problem, tile_rows):
        rowptr, truth_idx, idf32, sums32, v, n = problem
        out = np.zeros(8, dtype=np.uint64)
        pointer = lambda x: x.ctypes.data_as(ctypes.c_void_p)
        assert library.ds_index_image_digest(pointer(rowptr), pointer(truth_idx), pointer(idf32), pointer(sums32),
                                             ctypes.c_int64(v), ctypes.c_int64(n), ctypes.c_int64(tile_rows), pointer(out)) == 0
        return [int(word) for word in out]
    return digest


def _digests_agree(host_digest, monkeypatch, problem):
    for sort_rows in (True, False):
        if sort_rows:
            monkeypatch.delenv("DS_SORT_ROWS", raising=False)
        else:
            monkeypatch.setenv("DS_SORT_ROWS", "0")
        for tile_rows in TILE_ROWS:
            image = ic.expected_image(*problem[:4], tile_rows, sort_rows=sort_rows)
            assert ic.image_digest(image) == host_digest(problem, tile_rows), (sort_rows, tile_rows)


@pytest.mark.parametrize("name", sorted(SMALL))
def test_the_restated_image_is_the_hosts_on_named_problems(host_digest, monkeypatch, name):
    _digests_agree(host_digest, monkeypatch, SMALL[name]())


@pytest.mark.parametrize("shape,sums,size", GENERATED)
def test_the_restated_image_is_the_hosts_on_generated_problems(host_digest, monkeypatch, shape, sums, size):
    n_rows, n_columns, seed = size
    _digests_agree(host_digest, monkeypatch, ic.adversarial_problem(seed, n_rows, n_columns, shape, sums))


def test_the_generated_problems_cover_every_shape_and_sums():
    assert len(GENERATED) >= 40 and {(shape, sums) for shape, sums, _ in GENERATED} == {(a, b) for a in ic.SHAPES for b in ic.SUMS}


def test_the_image_has_the_names_types_and_shapes_of_truth_index_image():
    from doppel_speller_amd.match_maker import IMAGE_ARRAYS, IMAGE_SCALARS
    for problem, wide in ((ic.columns_at(65536), False), (ic.columns_at(65537), True), (ic.no_postings(5), False)):
        image = ic.expected_image(*problem[:4], 64)
        v, n = problem[4], problem[5]
        assert set(image) == set(IMAGE_ARRAYS) | set(IMAGE_SCALARS)
        for name, dtype in IMAGE_ARRAYS.items():
            widths = {"row_start": np.uint32, "row_cols": np.int32 if wide else np.uint16}
            assert image[name].dtype == (dtype or widths[name]), name
        assert image["col_ptr"].shape == (v, image["n_tiles"] + 1) and image["records"].shape == (n, 8)
        assert image["sums32"].shape == (n + 8,) and image["row_start"].shape == (n + 1,) and image["sig_column"].shape == (v,)
        assert image["postings"].shape == image["posting_sums"].shape == (4 * image["n_quads"],)
        assert image["row_cols"].shape == (int(problem[0][-1]),) and image["row_cols_bytes"] == (4 if wide else 2)
        assert all(isinstance(image[name], int) for name in IMAGE_SCALARS)


# ---- the generator ---------------------------------------------------------------------------------------------------
def test_generated_rows_and_queries_are_those_of_the_property_test():
    pytest.importorskip("hypothesis")
    import test_gpu_property as tp
    for seed, (shape, n_rows, n_columns) in enumerate((("random", 40, 30), ("twins", 300, 7), ("single", 90, 400), ("dense", 1, 1))):
        theirs = tp._problem(seed, n_rows, n_columns, shape, n_queries=12)
        rowptr, truth_idx, idf32, sums32, _, _ = ic.adversarial_problem(seed, n_rows, n_columns, shape, "true")
        queries = ic.adversarial_queries(seed, n_rows, n_columns, shape)
        for mine, name in zip((rowptr, truth_idx, idf32, sums32) + queries,
                              ("rowptr", "truth_idx", "idf32", "sums32", "q_rowptr", "q_cols", "q_maxint")):
            assert mine.dtype == theirs[name].dtype and mine.tobytes() == theirs[name].tobytes(), (shape, name)


@pytest.mark.parametrize("shape", ic.SHAPES)
def test_what_the_sums_of_a_generated_problem_hold(shape):
    n, v, seed = 120, 25, 77
    rowptr, truth_idx, idf32, true32, _, _ = ic.adversarial_problem(seed, n, v, shape, "true")
    assert ic.in_range(idf32).all() and ic.literal_only_rule(rowptr, truth_idx, idf32, true32) == 0
    assert np.array_equal(true32, ic.true_sums(rowptr, truth_idx, idf32, n))
    totals = ic.idf_totals(rowptr, truth_idx, idf32, n)
    for sums in ic.SUMS:     # the rows do not depend on the sums
        other = ic.adversarial_problem(seed, n, v, shape, sums)
        assert np.array_equal(other[0], rowptr) and np.array_equal(other[1], truth_idx) and np.array_equal(other[2], idf32)
    assert np.unique(ic.adversarial_problem(seed, n, v, shape, "equal")[3]).shape[0] == 1
    assert np.unique(ic.adversarial_problem(seed, n, v, shape, "few")[3]).shape[0] == 3
    specials = ic.adversarial_problem(seed, n, v, shape, "specials")[3]
    changed = np.nonzero(specials.view(np.uint32) != true32.view(np.uint32))[0]
    assert set(specials.view(np.uint32).tolist()) >= set(ic.SPECIAL_BITS.values()) and changed.shape[0] <= len(ic.SPECIAL_BITS)
    assert np.float32(1e30).view(np.uint32) == ic.SPECIAL_BITS["1e30"] and not ic.in_range(np.float32(1e30)) and \
        ic.in_range(np.uint32(ic.SPECIAL_BITS["below_1e30"]).view(np.float32)) and \
        0 < np.uint32(ic.SPECIAL_BITS["denormal"]).view(np.float32) < np.finfo(np.float32).tiny
    # edge_low: one row under the bound of the literal_only rule, one at the first float32 that is not
    edge = ic.adversarial_problem(seed, n, v, shape, "edge_low")[3]
    changed = np.nonzero(edge != true32)[0]
    bound = totals * (1.0 - 1e-4)
    under = changed[edge[changed].astype(np.float64) < bound[changed]]
    over = np.setdiff1d(changed, under)
    assert under.shape[0] == 1 and over.shape[0] == 1
    assert float(np.nextafter(edge[under[0]], np.float32(np.inf))) >= bound[under[0]]
    assert float(np.nextafter(edge[over[0]], np.float32(-np.inf))) < bound[over[0]] <= float(edge[over[0]])
    assert ic.literal_only_rule(rowptr, truth_idx, idf32, edge) == 1
    edge[under[0]] = true32[under[0]]
    assert ic.literal_only_rule(rowptr, truth_idx, idf32, edge) == 0


def test_sparse_rows_have_no_column_at_both_ends_of_the_internal_order():
    for sort_rows, sums in ((True, "equal"), (False, "true"), (False, "specials")):
        rowptr, truth_idx, _, sums32, _, n = ic.adversarial_problem(3, 250, 60, "sparse", sums)
        p_rowptr, p_idx, _, _ = ic.internal_csr(rowptr, truth_idx, sums32, sort_rows)
        lengths = np.diff(ic.forward_lists(p_rowptr, p_idx, n)[0])
        assert lengths[0] == lengths[1] == lengths[-2] == lengths[-1] == 0 and 0 < (lengths > 0).sum() < n // 3
    # sorted by true sums the rows without a column come first (sums32 0.0)
    rowptr, truth_idx, _, sums32, _, n = ic.adversarial_problem(3, 250, 60, "sparse", "true")
    p_rowptr, p_idx, _, _ = ic.internal_csr(rowptr, truth_idx, sums32)
    lengths = np.diff(ic.forward_lists(p_rowptr, p_idx, n)[0])
    assert (lengths[:(lengths == 0).sum()] == 0).all()
    assert int(ic.adversarial_problem(3, 2, 60, "sparse", "true")[0][-1]) == 0          # one or two rows: no posting at all


# ---- the named problems ----------------------------------------------------------------------------------------------
def test_one_and_no_postings():
    rowptr, truth_idx, idf32, sums32, v, n = ic.one()
    assert (v, n, int(rowptr[-1]), truth_idx.shape[0]) == (1, 1, 1, 1) and ic.bits_of(1) == 1 and ic.sort_passes(1) == 1
    for n in ic.NO_POSTINGS:
        rowptr, truth_idx, idf32, sums32, v, rows = ic.no_postings(n)
        assert (v, rows) == (3, n) and not rowptr.any() and truth_idx.shape[0] == 0
        assert ic.literal_only_rule(rowptr, truth_idx, idf32, sums32) == 0
        ranks = ic.duplicate_ranks_rule(rowptr, truth_idx, sums32)
        for value in np.unique(sums32):      # every row is a twin of the rows with its sums32
            assert np.array_equal(np.sort(ranks[sums32 == value]), np.arange((sums32 == value).sum()))
        image = ic.expected_image(rowptr, truth_idx, idf32, sums32, 64)
        assert image["n_quads"] == 0 and not image["col_ptr"].any() and not image["row_start"].any()
        assert (image["sig_column"] == -1).all() and not image["records"][:, :4].any()
    rowptr, truth_idx, _, sums32, _, _ = ic.no_postings(65537, values=(1.0,))      # one group: the ranks saturate
    assert np.array_equal(ic.duplicate_ranks_rule(rowptr, truth_idx, sums32), np.minimum(np.arange(65536, -1, -1), 65535))


@pytest.mark.parametrize("n", ic.ROWS_AT)
def test_rows_at(n):
    rowptr, truth_idx, idf32, sums32, v, rows = ic.rows_at(n)
    assert (v, rows) == (9, n) and truth_idx.max() == n - 1 and (n < 60 or 2.5 < rowptr[-1] / n < 3.5)
    assert ic.sort_passes(n) == (1 if n <= 256 else 2 if n <= 65536 else 3)
    assert ic.literal_only_rule(rowptr, truth_idx, idf32, sums32) == 0


@pytest.mark.parametrize("v", ic.COLUMNS_AT)
def test_columns_at(v):
    rowptr, truth_idx, idf32, sums32, columns, n = ic.columns_at(v)
    lengths = np.diff(rowptr)
    assert (columns, n) == (v, 500) and ic.sort_passes(v) == (1 if v <= 256 else 2 if v <= 65536 else 3)
    assert all(lengths[c] > 0 for c in (0, v - 1, 65535, 65536) if c < v)
    assert ic.literal_only_rule(rowptr, truth_idx, idf32, sums32) == 0
    # the density cut at 500 rows is a length of 2, and the columns of that length are a tie of at least 130 (or all)
    assert 2 * 256 >= n > 1 * 256 and (lengths == 2).sum() >= min(v, 130)
    sig_column = ic.signature_columns(rowptr, n)
    assert (sig_column >= 0).sum() == min(128, (lengths >= 2).sum()) and not (sig_column[lengths < 2] >= 0).any()
    if v >= 129:      # the bits run out inside the tie: the lower columns of it get them
        tied = np.nonzero(lengths == 2)[0]
        with_bit = tied[sig_column[tied] >= 0]
        assert 0 < with_bit.shape[0] < tied.shape[0] and with_bit.max() < tied[sig_column[tied] < 0].min()
        assert sig_column[0] >= 0 and sig_column[v - 1] == -1
    image = ic.expected_image(rowptr, truth_idx, idf32, sums32, ic.NARROW)
    assert image["row_cols"].dtype == (np.uint16 if v <= 65536 else np.int32) and image["row_cols"].max() == v - 1


@pytest.mark.parametrize("m", ic.POSTINGS_AT)
def test_postings_at(m):
    rowptr, truth_idx, idf32, sums32, v, n = ic.postings_at(m)
    assert int(rowptr[-1]) == m == truth_idx.shape[0] and ic.literal_only_rule(rowptr, truth_idx, idf32, sums32) == 0
    # a scan of m + 1 entries in workgroups of 2048: the end entry is alone in the last one when m is a multiple
    assert ((m + 1) % 2048 == 1) == (m in (2048, 4096))


@pytest.mark.parametrize("t", [ic.NARROW, ic.WIDE])
def test_tile_edges(t):
    for n, (n_tiles, last) in zip(ic.tile_edge_rows(t), ((1, t - 1), (1, t), (2, 1), (2, t), (3, 1))):
        rowptr, truth_idx, idf32, sums32, v, rows = ic.tile_edges(n, t)
        assert rows == n and (n + t - 1) // t == n_tiles and n - (n_tiles - 1) * t == last
        assert np.array_equal(ic.internal_csr(rowptr, truth_idx, sums32)[3], np.arange(n))      # the caller's order
        assert np.array_equal(truth_idx[rowptr[0]:rowptr[1]], np.arange(n))
        assert truth_idx[rowptr[1]:rowptr[2]].tolist() == [r for r in (t - 1, t) if r < n]
        assert ic.literal_only_rule(rowptr, truth_idx, idf32, sums32) == 0


@pytest.mark.parametrize("t", [64, ic.NARROW, ic.WIDE])
def test_nan_tiles(t):
    rowptr, truth_idx, idf32, sums32, v, n = ic.nan_tiles(t)
    assert n == t + 5
    nan = np.isnan(sums32)
    # sorted: the -NaN first, the last tile all +NaN
    p_sums = ic.internal_csr(rowptr, truth_idx, sums32)[2]
    assert p_sums.view(np.uint32)[0] == 0xffc00000 and p_sums.view(np.uint32)[t:].tolist() == [0x7fc00000 + i for i in range(5)]
    assert not np.isnan(p_sums[1:t]).any()
    low, high, sums_min = ic.tile_bounds_rule(p_sums, t)
    assert low.view(np.uint32).tolist() == high.view(np.uint32).tolist() == [0xffc00000, 0x7fc00000]
    assert sums_min.view(np.uint32)[0] == 0xffc00000
    # the caller's order: a NaN starts tile 1, NaNs lie inside both tiles, the zeros are tile 0's smallest values
    assert nan[t] and nan[t + 2] and not nan[0] and nan[1:t].sum() == 4 and nan[t + 1:].sum() == 1
    zeros = np.nonzero(sums32 == 0)[0]
    assert zeros.tolist() == [10, 20, 30, 40] and sums32.view(np.uint32)[zeros].tolist() == [0x80000000, 0, 0x80000000, 0]
    assert np.nanmin(sums32) == 0
    low, high, sums_min = ic.tile_bounds_rule(sums32, t)
    assert low.view(np.uint32).tolist() == [0x80000000, 0x7fc00000] and high.view(np.uint32)[1] == 0x7fc00000     # first of equals
    assert high[0] == np.nanmax(sums32[:t]) and sums_min.view(np.uint32)[0] == 0x80000000
    assert ic.literal_only_rule(rowptr, truth_idx, idf32, sums32) == 1


@pytest.mark.parametrize("bad_row", [4999, 2500])
def test_one_bad_row(bad_row):
    rowptr, truth_idx, idf32, sums32, v, n = ic.one_bad_row(bad_row)
    true32 = ic.true_sums(rowptr, truth_idx, idf32, n)
    assert n == 5000 and np.nonzero(sums32 != true32)[0].tolist() == [bad_row]
    assert ic.in_range(idf32).all() and ic.in_range(sums32).all()
    assert ic.literal_only_rule(rowptr, truth_idx, idf32, sums32) == 1
    assert ic.literal_only_rule(rowptr, truth_idx, idf32, true32) == 0          # repaired


@pytest.mark.parametrize("hash_bits", ic.HASH_BITS)
def test_stray_largest(hash_bits):
    rowptr, truth_idx, _, sums32, v, n = ic.stray_largest(hash_bits)
    p_rowptr, p_idx, p_sums, _ = ic.internal_csr(rowptr, truth_idx, sums32)
    groups, lists = ic.hash_groups(p_rowptr, p_idx, p_sums, hash_bits)
    assert len(groups) == 40 and all(len(members) == 5 for members in groups)
    stray = [members for members in groups if all(lists[t] != lists[members[-1]] for t in members[:-1])]
    assert len(stray) >= 10 and (hash_bits + 7) // 8 == (2 if hash_bits == 9 else 1)
    cut = ic.duplicate_ranks_rule(p_rowptr, p_idx, p_sums, hash_bits)
    whole = ic.duplicate_ranks_rule(p_rowptr, p_idx, p_sums)
    assert all(not cut[members].any() and sorted(whole[members].tolist()) == [0, 0, 1, 2, 3] for members in stray)
    mixed = [members for members in groups if members not in stray]
    assert all(sorted(cut[members].tolist()) == [0, 0, 0, 1, 2] and sorted(whole[members].tolist()) == [0, 0, 1, 1, 2]
               for members in mixed) and len(mixed) == 20
