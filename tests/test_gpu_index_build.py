"""The index built on the device (ds_index_create_device) against the host's image (ds_index_create): every array of
ds_index_read, the scalar fields and ds_index_info, byte for byte, on inputs that put each stage of the build at its
edges; the refusals of the validation stage; the duplicate ranks under truncated hashes against the NumPy restatement of
the rule (index_build_cases.duplicate_ranks_rule, pinned on the CPU by test_index_build_cpu.py); and the index in use:
ds_jaccard_topk against oracle.jaccard_topk, Prediction and duplicate_groups against their host-built twins."""
import ctypes

import numpy as np
import pytest

import index_build_cases as ic
import jaccard_cases as jc

pytestmark = pytest.mark.gpu
ARRAYS = ("col_ptr", "postings", "posting_sums", "records", "sums32", "tile_sums_min", "tile_sums_max", "sig_column",
          "row_start", "row_cols", "idf32")
SCALARS = ("n_tiles", "n_quads", "sums_min_bits", "literal_only", "rows_sorted", "row_start_bytes", "row_cols_bytes",
           "tile_rows")


def _build(arrays, build, geometry=None, sort_rows=None):
    """A TruthIndex of (rowptr, truth_idx, idf32, sums32, ...) with the environment set around the create call."""
    import doppel_speller_amd as ds
    with pytest.MonkeyPatch.context() as patch:
        if geometry is not None:
            patch.setenv("DS_GEOMETRY", geometry)
        if sort_rows is not None:
            patch.setenv("DS_SORT_ROWS", "1" if sort_rows else "0")
        return ds.TruthIndex(*arrays[:4], build=build)


def _same_image(host, device):
    """Every array and scalar of the two indexes; returns the host's image."""
    expected, got = host.image(), device.image()
    assert host.info() == device.info()
    for name in SCALARS:
        assert expected[name] == got[name], (name, expected[name], got[name])
    for name in ARRAYS:
        a, b = expected[name], got[name]
        assert a.dtype == b.dtype and a.shape == b.shape, (name, a.dtype, b.dtype, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            differ = np.nonzero(a.reshape(-1).view(np.uint8) != b.reshape(-1).view(np.uint8))[0]
            raise AssertionError((name, "bytes differ", differ.shape[0], "first at byte", int(differ[0]),
                                  a.reshape(-1)[differ[0] // a.itemsize], b.reshape(-1)[differ[0] // a.itemsize]))
    return expected


def _both(arrays, **environment):
    host, device = _build(arrays, "host", **environment), _build(arrays, "device", **environment)
    return host, device, _same_image(host, device)


# ---- 1. both geometries on synthetic rows ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def synthetic():
    from doppel_speller_amd import synth
    made = {}

    def workload(n_truth):
        if n_truth not in made:
            w = synth.make_workload(n_truth, 16)
            made[n_truth] = (w.rowptr, w.truth_idx, w.idf32, w.sums32, w)
        return made[n_truth]
    return workload


@pytest.mark.parametrize("n_truth,geometry,sort_rows", [(2 * ic.NARROW + 1, "narrow", True), (2 * ic.WIDE + 1, "wide", True),
                                                        (2 * ic.NARROW + 1, "narrow", False)])
def test_synthetic_rows_in_both_geometries(synthetic, n_truth, geometry, sort_rows):
    _, _, image = _both(synthetic(n_truth), geometry=geometry, sort_rows=sort_rows)
    assert image["n_tiles"] == 3 and image["tile_rows"] == (ic.NARROW if geometry == "narrow" else ic.WIDE)
    assert image["rows_sorted"] == int(sort_rows) and image["literal_only"] == 0


# ---- 2. hand-made CSR: part edges, empty and full columns, ties, signs -----------------------------------------------
@pytest.mark.parametrize("sums,full_column", [("equal", True), ("equal", False), ("runs", True), ("runs", False),
                                              ("signed", True)])
def test_part_edges_ties_and_signs(sums, full_column):
    arrays = ic.part_edges_problem(sums, full_column)
    _, _, image = _both(arrays, geometry="narrow")
    assert image["n_tiles"] == 3
    if sums == "equal":      # the stable tie rule alone: the internal order is the caller's
        assert np.array_equal(image["records"][:, 6], np.arange(arrays[5], dtype=np.uint32))
    if sums == "signed":
        assert image["literal_only"] == 1
        assert np.array_equal(image["records"][:, 6], np.argsort(ic.order_key(arrays[3]), kind="stable").astype(np.uint32))


# ---- 3. duplicate ranks ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def twins():
    arrays = ic.twins_problem()
    internal = ic.internal_csr(arrays[0], arrays[1], arrays[3])
    return arrays, internal


def test_duplicate_ranks_saturate_and_cross_a_tile_boundary(twins):
    arrays, (p_rowptr, p_idx, p_sums, original) = twins
    _, _, image = _both(arrays)
    ranks = image["records"][:, 5]
    assert np.array_equal(image["records"][:, 6], original.astype(np.uint32))
    assert np.array_equal(ranks, ic.duplicate_ranks_rule(p_rowptr, p_idx, p_sums).astype(np.uint32))
    assert ranks.max() == 65535 and int((ranks == 65535).sum()) == 70000 - 65535
    # the 600 twins lie across the boundary of tiles 5 and 6; the 50 rows with the same set and other bits are not theirs
    six_hundred = np.nonzero(p_sums.view(np.uint32) == np.float32(12).view(np.uint32))[0]
    assert six_hundred[0] < 6 * ic.NARROW <= six_hundred[-1] and six_hundred.shape[0] == 600
    assert np.array_equal(np.sort(ranks[six_hundred]), np.arange(600))
    others = np.nonzero(p_sums == np.nextafter(np.float32(12), np.float32(13)))[0]
    assert np.array_equal(np.sort(ranks[others]), np.arange(50))


def test_truncated_hashes_follow_the_rule_and_the_default_comes_back(twins):
    import doppel_speller_amd as ds
    arrays, (p_rowptr, p_idx, p_sums, _) = twins
    option = ds._lib.lib().ds_index_build_option
    plain = ic.duplicate_ranks_rule(p_rowptr, p_idx, p_sums)
    cut = ic.duplicate_ranks_rule(p_rowptr, p_idx, p_sums, hash_bits=2)
    assert not np.array_equal(plain, cut)
    assert option(b"duplicate_hash_bits", 2) == 0
    try:
        ranks = _build(arrays, "device").image()["records"][:, 5]
    finally:
        assert option(b"duplicate_hash_bits", 0) == 0
    assert np.array_equal(ranks, cut.astype(np.uint32))
    _both(arrays)      # back at 0: the host's again


# ---- 4. wide columns -------------------------------------------------------------------------------------------------
def test_more_than_65536_columns():
    _, _, image = _both(ic.wide_columns_problem())
    assert image["row_cols_bytes"] == 4 and image["row_cols"].dtype == np.int32 and image["row_cols"].max() == 69999


# ---- 5. refusals -----------------------------------------------------------------------------------------------------
def test_refusals_and_a_valid_build_after_them():
    import doppel_speller_amd as ds
    library, pointer = ds._lib.lib(), ds._lib.pointer
    for name, (rowptr, idx, idf32, sums32, v, n, needle) in ic.refused_inputs().items():
        outcome = []
        for create in (library.ds_index_create, library.ds_index_create_device):
            out = ctypes.c_void_p(1)
            status = create(pointer(rowptr), pointer(idx), pointer(idf32), pointer(sums32), v, n, 0, ctypes.byref(out))
            outcome.append((status, library.ds_last_error(), out.value))
        assert outcome[0] == outcome[1], (name, outcome)
        assert outcome[1][0] == -1 and needle in outcome[1][1] and outcome[1][2] is None, (name, outcome)
    _both(ic.part_edges_problem("runs", False), geometry="narrow")


def test_index_read_sizes_and_refuses():
    import doppel_speller_amd as ds
    library = ds._lib.lib()
    index = _build(ic.wide_columns_problem(), "device")
    size = ctypes.c_size_t(7)
    assert library.ds_index_read(index.handle, b"no_such_array", None, 0, ctypes.byref(size)) == -1 and size.value == 0
    assert library.ds_index_read(index.handle, b"idf32", None, 0, ctypes.byref(size)) == -1 and size.value == 4 * 70000
    small = np.zeros(10, dtype=np.float32)
    assert library.ds_index_read(index.handle, b"idf32", ds._lib.pointer(small), small.nbytes, ctypes.byref(size)) == -1
    assert size.value == 4 * 70000 and not small.any()


# ---- 6. the index is usable ------------------------------------------------------------------------------------------
def _topk_equals_oracle(oracle, case, geometry):
    rowptr, truth_idx, idf32, sums32, q_rowptr, q_cols, q_maxint, k = jc.arrays(case)
    index = _build((rowptr, truth_idx, idf32, sums32), "device", geometry=geometry)
    assert index.info()["tile_rows"] == jc.GEOMETRY[geometry]["tile_rows"]
    rows = index.top_k(q_rowptr, q_cols, q_maxint, k)
    assert index.sync()["error_queries"] == 0
    assert np.array_equal(rows, oracle.jaccard_topk(*jc.arrays(case)))


@pytest.mark.parametrize("geometry", jc.GEOMETRIES)
def test_jaccard_cases_on_a_device_built_index(oracle, geometry):
    _topk_equals_oracle(oracle, dict(jc.tie_problem(geometry), k=jc.k_class_edges(geometry)[1]), geometry)
    _topk_equals_oracle(oracle, jc.descending_epochs_problem(geometry), geometry)


@pytest.mark.parametrize("geometry", jc.GEOMETRIES)
def test_synthetic_workload_on_a_device_built_index(oracle, geometry):
    from doppel_speller_amd import synth
    w = synth.make_workload(30000, 257)
    for k in (10, 100):
        _topk_equals_oracle(oracle, dict(rowptr=w.rowptr, truth_idx=w.truth_idx, idf32=w.idf32, sums32=w.sums32,
                                         q_rowptr=w.q_rowptr, q_cols=w.q_cols, q_maxint=w.q_maxint, k=k), geometry)


def test_prediction_and_duplicate_groups_do_not_depend_on_the_build():
    import doppel_speller_amd as ds
    from doppel_speller_amd import synth
    w = synth.make_workload(5000, 500)
    truth, queries = synth._to_strings(w.t_flat, w.t_off), synth._to_strings(w.q_flat, w.q_off)
    forest = synth.make_forest(n_trees=50)
    model = ds.ForestModel(forest["feature"], forest["threshold"], forest["yes"], forest["no"], forest["missing"],
                           forest["tree_offsets"], forest["n_features"], forest["base_margin"])
    answers = {}
    for build in ("host", "device"):
        p = ds.Prediction(truth, w.title_id, model, top_n=10, transform=False, build_index=build)
        assert p.index.build == build and p.index_build_ms > 0
        frame = p.generate_test_predictions(queries)
        answers[build] = (frame, p.details, p.duplicate_groups())
    for host, device in zip(answers["host"], answers["device"]):
        assert list(host.columns) == list(device.columns) and len(host) == len(device)
        for column in host.columns:
            assert np.array_equal(host[column].to_numpy(), device[column].to_numpy(), equal_nan=host[column].dtype.kind == "f"), column
    assert (answers["host"][0]["title_id"] >= 0).sum() > 100


# ---- 7. repetition ---------------------------------------------------------------------------------------------------
def test_two_device_builds_give_the_same_image():
    arrays = ic.part_edges_problem("signed")
    _same_image(_build(arrays, "device", geometry="narrow"), _build(arrays, "device", geometry="narrow"))
