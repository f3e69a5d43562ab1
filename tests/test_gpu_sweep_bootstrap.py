"""The bootstrap of the sweep's cells on the GPU ("Bootstrap of the cells"; csrc/ds_sweep.hip)
against tests/sweep_bootstrap_oracle.py.  Everything is an integer, so everything is compared with ==: the records of
ds_sweep_records_device, the counts of ds_sweep_bootstrap_device under every tiling and grid the launcher has, its
refusals, and Prediction.threshold_sweep(n_boot=) against bootstrap_accuracy cell by cell."""
import contextlib

import numpy as np
import pytest

import bootstrap_oracle as bo
import sweep_bootstrap_oracle as so

pytestmark = pytest.mark.gpu

DEFAULTS = dict(bootstrap_tile=0, bootstrap_max_blocks=0, bootstrap_replicates_per_group=0, queries_per_group=0)


@contextlib.contextmanager
def options(**values):
    """ds_sweep_option for the duration of a block; every option is back at its default afterwards."""
    from doppel_speller_amd import _lib
    try:
        for name, value in values.items():
            _lib.check(_lib.lib().ds_sweep_option(name.encode(), value), "ds_sweep_option")
        yield
    finally:
        for name in values:
            _lib.lib().ds_sweep_option(name.encode(), DEFAULTS[name])


def device_records(c, fill=0xffff):
    """ds_sweep_records_device on a record_case -> (status, uint16[Q][T])."""
    from doppel_speller_amd import _lib
    rows, d, r, s, p, exact, actual = c["queries"]
    held = [_lib.DeviceArray.from_host(a) for a in (rows, d, r, s, p, exact, actual, c["lev"], c["prob"])]
    out = _lib.DeviceArray.from_host(np.full((rows.shape[0], len(c["lev"])), fill, np.uint16))
    try:
        status = _lib.lib().ds_sweep_records_device(*(a.ptr for a in held[:7]), rows.shape[0], rows.shape[1], held[7].ptr,
                                                    len(c["lev"]), held[8].ptr, len(c["prob"]), out.ptr)
        return status, out.to_host()
    finally:
        for array in held + [out]:
            array.free()


def device_bootstrap(records, T, U, unit, n_units, n_boot, seed, fill=-7):
    """ds_sweep_bootstrap_device -> (status, counts, baseline); the outputs start as `fill`."""
    from doppel_speller_amd import _lib
    records = np.ascontiguousarray(records, dtype=np.uint16)
    d_records = _lib.DeviceArray.from_host(records)
    d_unit = None if unit is None else _lib.DeviceArray.from_host(np.ascontiguousarray(unit, dtype=np.int32))
    d_counts = _lib.DeviceArray.from_host(np.full((n_boot, T, U, 4), fill, np.int64))
    d_baseline = _lib.DeviceArray.from_host(np.full((T, U, 4), fill, np.int64))
    try:
        status = _lib.lib().ds_sweep_bootstrap_device(d_records.ptr, records.shape[0], T, U, _lib.pointer(d_unit), n_units,
                                                      n_boot, seed, d_counts.ptr, d_baseline.ptr)
        return status, d_counts.to_host(), d_baseline.to_host()
    finally:
        for array in (d_records, d_unit, d_counts, d_baseline):
            if array is not None:
                array.free()


# ---- 1. the records ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_queries, k, grid", so.RECORD_CASES)
def test_records_equal_the_oracle(oracle, n_queries, k, grid):
    """Q = 1, 4, 5 and 257 leave a workgroup's four waves partly idle; k crosses the 64 candidates a wave loads at a
    time; T = 64 and 65 the 64 thresholds of a tile; U = 46, 47 and 256 the tile edges of the counting kernel."""
    c = so.record_case(oracle, n_queries, k, grid)
    status, records = device_records(c)
    assert status == 0
    assert records.tobytes() == c["records"].tobytes()
    with options(queries_per_group=4):
        assert device_records(c)[1].tobytes() == c["records"].tobytes()


def test_the_cases_hold_every_kind_of_record(oracle):
    """Asserted on the oracle's records.  A flip is read off the codes, so it lies before the last cell: its pos is in
    1..U - 1 (a model maximum above every threshold of the grid is the same outcome in every cell, and both the oracle
    and the kernel write that outcome; the 3 x 7 cases hold such titles: probabilities of 1.0 above the last threshold
    0.99).  pos = U is a record the bootstrap kernel takes all the same: test_a_pos_of_u_counts_as_matched_everywhere."""
    for n_queries, k, grid in ((257, 65, "3x7"), (257, 64, "65x47"), (257, 5, "64x46"), (5, 65, "101x256")):
        c = so.record_case(oracle, n_queries, k, grid)
        what, pos = c["records"] & 7, c["records"] >> 3
        U = len(c["prob"])
        if n_queries == 257:
            assert set(np.unique(what).tolist()) == {0, 1, 2, 3, 4, 5, 6}, grid
            assert (pos[what >= 4] == 1).any() and (pos[what >= 4] == U - 1).any(), grid
        assert (what >= 4).any(), grid
    rows, _, _, _, p, exact, _ = so.record_case(oracle, 257, 65, "3x7")["queries"]
    top = np.sort(p, axis=1)
    assert ((top[:, -1] == 1.0) & (top[:, -2] < 1.0) & (exact < 0)).any()        # a maximum above every threshold


# ---- 2. the resampling ----------------------------------------------------------------------------------------------------
FORMS = (dict(bootstrap_tile=1), dict(bootstrap_tile=3), dict(bootstrap_tile=64), dict(bootstrap_max_blocks=1),
         dict(bootstrap_max_blocks=3), dict(bootstrap_replicates_per_group=1), dict(bootstrap_replicates_per_group=7),
         dict(bootstrap_tile=2, bootstrap_max_blocks=1, bootstrap_replicates_per_group=11),
         dict(bootstrap_tile=5, bootstrap_max_blocks=2, bootstrap_replicates_per_group=3))


@pytest.mark.parametrize("n_boot", [1, 5])
@pytest.mark.parametrize("n_units", so.UNITS)
@pytest.mark.parametrize("n, grid", so.BOOT_CASES)
def test_counts_equal_the_oracle_in_every_form(oracle, n, grid, n_units, n_boot):
    """Records taken from the oracle; without units and with 1 unit (it holds every title), 2 (one holds every title,
    one is empty) and 65 (the last is empty); a seed that uses its high half.  The launcher has one form of the kernel
    per unit mode, all counters in LDS; what it chooses is the thresholds per tile, the grid's cap and the replicates per
    workgroup, and every one of them must give the same arrays.  No counter is narrower than 32 bits."""
    c = so.boot_case(oracle, n, grid, n_units, n_boot)
    assert c["seed"] >> 32

    def same(form):
        status, counts, baseline = device_bootstrap(c["records"], c["T"], c["U"], c["unit"], c["n_units"], n_boot, c["seed"])
        assert status == 0, form
        assert counts.tobytes() == c["counts"].tobytes(), form
        assert baseline.tobytes() == c["baseline"].tobytes(), form
    same("default")
    for form in FORMS if c["T"] * c["U"] <= 1000 else FORMS[1::3]:
        with options(**form):
            same(form)


def test_more_titles_than_sixteen_bits_count(oracle):
    """70,001 titles with the same record (right below pos 1, not found from there), T = 1, U = 2, B = 2: every counter
    that is not 0 is 70,001, in every replicate, whatever is drawn."""
    records = np.full((70001, 1), 5 | (1 << 3), np.uint16)
    status, counts, baseline = device_bootstrap(records, 1, 2, None, 70001, 2, 12345)
    assert status == 0
    assert baseline.tolist() == [[[0, 0, 0, 70001], [0, 0, 70001, 0]]]
    assert counts.tolist() == [baseline.tolist()] * 2
    with options(bootstrap_max_blocks=1):
        assert device_bootstrap(records, 1, 2, None, 70001, 2, 12345)[1].tolist() == counts.tolist()


def test_a_pos_of_u_counts_as_matched_everywhere(oracle):
    """The fixed matched outcomes of the oracle's records rewritten as flips with pos = U: the same counts."""
    c = so.boot_case(oracle, 257, "3x7", 65, 5)
    records = c["records"].copy()
    records[c["records"] == 3] = 5 | (c["U"] << 3)
    ones = np.argwhere(c["records"] == 1)
    for at, (q, t) in enumerate(ones):
        records[q, t] = (4 if at % 2 else 6) | (c["U"] << 3)
    assert (records >> 3 == c["U"]).sum() > 100 and np.array_equal(so.decode(records, c["U"]), c["codes"])
    status, counts, baseline = device_bootstrap(records, c["T"], c["U"], c["unit"], c["n_units"], 5, c["seed"])
    assert status == 0 and counts.tobytes() == c["counts"].tobytes() and baseline.tobytes() == c["baseline"].tobytes()


def test_the_largest_replicate_must_fit_32_bits():
    """65,536 units, one of them with 65,536 titles: a replicate could add 2^32 titles to one counter, and the call is
    refused; with one unit less it runs, and a replicate's count is the sum of the sizes of the drawn units."""
    from doppel_speller_amd import _lib
    unit = np.concatenate([np.zeros(65536, np.int32), np.arange(1, 65536, dtype=np.int32)])
    records = np.ones((unit.shape[0], 1), np.uint16)
    status, counts, baseline = device_bootstrap(records, 1, 1, unit, 65536, 1, 9)
    assert status == -1 and b"2^32" in _lib.lib().ds_last_error()
    assert (counts == -7).all() and (baseline == -7).all()
    unit = unit[:-1]
    status, counts, baseline = device_bootstrap(records[:-1], 1, 1, unit, 65535, 1, 9)
    assert status == 0 and baseline.reshape(-1).tolist() == [0, unit.shape[0], 0, 0]
    sizes = np.bincount(unit, minlength=65535)
    assert counts.reshape(-1).tolist() == [0, int(sizes[bo.draws(9, 0, 65535)].sum()), 0, 0]


@pytest.mark.parametrize("what", ["low bits 7", "pos 0 on a flip", "pos U + 1", "pos on a fixed outcome", "unit -1",
                                  "unit n_units"])
def test_refusals_leave_the_counts_untouched(oracle, what):
    from doppel_speller_amd import _lib
    c = so.boot_case(oracle, 257, "3x7", 65, 5)
    records, unit = c["records"].copy(), c["unit"].copy()
    if what == "low bits 7":
        records[200, 2] = 7 | (1 << 3)
    elif what == "pos 0 on a flip":
        records[0, 0] = 5
    elif what == "pos U + 1":
        records[256, 1] = 6 | ((c["U"] + 1) << 3)
    elif what == "pos on a fixed outcome":
        records[3, 1] = 2 | (1 << 3)
    elif what == "unit -1":
        unit[100] = -1
    else:
        unit[256] = c["n_units"]
    status, counts, baseline = device_bootstrap(records, c["T"], c["U"], unit, c["n_units"], 5, c["seed"])
    assert status == -1
    message = _lib.lib().ds_last_error()
    assert (b"1 units are outside" if what.startswith("unit") else b"1 records are none") in message, message
    assert (counts == -7).all() and (baseline == -7).all()
    # and the scalars: U and T past their limits, n_boot outside 1..65,536, n_units != n without units
    d = _lib.DeviceArray.from_host(c["records"])
    try:
        for T, U, n_units, n_boot in ((c["T"], 257, 257, 5), (102, c["U"], 257, 5), (c["T"], c["U"], 257, 0),
                                      (c["T"], c["U"], 257, 65537), (c["T"], c["U"], 256, 5)):
            assert _lib.lib().ds_sweep_bootstrap_device(d.ptr, 257, T, U, None, n_units, n_boot, 1, d.ptr, d.ptr) == -1
    finally:
        d.free()


def test_no_titles_give_zeros():
    status, counts, baseline = device_bootstrap(np.zeros((0, 3), np.uint16), 3, 7, None, 0, 2, 1)
    assert status == 0 and not counts.any() and not baseline.any()


# ---- 3. through Prediction --------------------------------------------------------------------------------------------------
TOP_N = 10
LEVENSHTEIN = [80, 94, 97]
N_BOOT = 25
SEED = (77 << 32) + 5


@pytest.fixture(scope="module")
def problem():
    """The problem of tests/test_gpu_threshold_sweep.py, built the same way: 20,000 truth titles under permuted ids, 400
    titles, 40 % of them with no match, a forest, and probability thresholds between the model's own maxima."""
    import doppel_speller_amd as ds
    from doppel_speller_amd import synth
    w = synth.make_workload(20000, 400)
    truth = synth._to_strings(w.t_flat, w.t_off)
    ids = w.title_id
    queries = synth._to_strings(w.q_flat, w.q_off)
    actual_row = w.actual_row.copy()
    rng = np.random.RandomState(5)
    for q in rng.permutation(400)[:20]:
        actual_row[q] = rng.randint(0, 20000)
        queries[q] = truth[actual_row[q]]
    actual = np.where(actual_row >= 0, ids[np.maximum(actual_row, 0)], -1).astype(np.int64)
    forest = synth.make_forest(n_trees=100)
    model = ds.ForestModel(forest["feature"], forest["threshold"], forest["yes"], forest["no"], forest["missing"],
                           forest["tree_offsets"], forest["n_features"], forest["base_margin"])
    p = ds.Prediction(truth, ids, model, top_n=TOP_N, transform=False)
    p.ranked_matches(queries, n=1, keep_candidates=True)
    undecided = (p.candidates.exact < 0) & (p.candidates.close < 0)
    maxima = np.unique(p.candidates.probabilities[undecided].max(axis=1))
    assert maxima.shape[0] >= 8
    cuts = [float((maxima[at] + maxima[at + 1]) / 2) for at in (len(maxima) // 4, len(maxima) // 2)]
    return truth, ids, queries, actual, model, sorted(cuts + [0.9, float(maxima[len(maxima) // 3])])


@pytest.fixture(scope="module")
def swept(problem):
    """(Prediction, plain frame and timings, then per groups: frame, SweepBootstrap, timings)."""
    import doppel_speller_amd as ds
    truth, ids, queries, actual, model, probabilities = problem
    p = ds.Prediction(truth, ids, model, top_n=TOP_N, transform=False)
    plain = p.threshold_sweep(queries, actual, LEVENSHTEIN, probabilities)
    out = {"plain": (plain, dict(p.timings), p.sweep_bootstrap)}
    for name, groups in (("titles", None), ("ids", actual)):
        frame = p.threshold_sweep(queries, actual, LEVENSHTEIN, probabilities, n_boot=N_BOOT, groups=groups, seed=SEED)
        out[name] = (frame, p.sweep_bootstrap, dict(p.timings))
    return p, out


def _same_frame(a, b):
    return list(a.columns) == list(b.columns) and a.dtypes.tolist() == b.dtypes.tolist() and all(
        np.array_equal(a[c].to_numpy(), b[c].to_numpy()) for c in a.columns)


def test_the_frame_is_unchanged_and_the_baseline_is_its_counters(problem, swept):
    from doppel_speller_amd import bootstrap, prediction
    probabilities = problem[5]
    _, out = swept
    plain, plain_timings, plain_boot = out["plain"]
    assert plain_boot is None
    assert {"top_k", "close_parts", "exact_matches", "features", "model", "sweep", "copy_back", "host_prepare",
            "prepare_queries"} == set(plain_timings)
    for name in ("titles", "ids"):
        frame, boot, timings = out[name]
        assert _same_frame(plain, frame)
        assert isinstance(boot, bootstrap.SweepBootstrap) and boot.n_boot == N_BOOT and boot.seed == SEED
        assert boot.counts.shape == (N_BOOT, 12, 4) and boot.counts.dtype == np.int64
        assert boot.levenshtein_thresholds.tolist() == LEVENSHTEIN and boot.probability_thresholds.tolist() == probabilities
        assert np.array_equal(boot.baseline_counts, frame[[*bootstrap.ACCURACY_CODES]].to_numpy())
        assert np.array_equal(boot.baseline_errors, frame["custom_error"].to_numpy())
        assert set(timings) == set(plain_timings) | {"sweep_records", "sweep_bootstrap"}
        assert timings["sweep_records"] > 0 and timings["sweep_bootstrap"] > 0
        assert _same_frame(boot.frame()[list(prediction.SWEEP_COLUMNS)], frame)
        assert abs(boot.share_best.sum() - 1) < 1e-12 and boot.reference == (94, 0.9)
        assert boot.against()["baseline"].tolist() == (boot.baseline_errors - boot.baseline_errors[boot.cell(94, 0.9)]).tolist()
    assert out["titles"][1].n_units == 400 and out["ids"][1].n_units == len(set(problem[3].tolist()))
    assert not np.array_equal(out["titles"][1].counts, out["ids"][1].counts)


@pytest.mark.parametrize("t, u_index", [(94, None), (80, 0), (94, 3)])
def test_a_cell_is_bootstrap_accuracy_of_generate_test_predictions_there(problem, swept, t, u_index):
    """Bit for bit, with and without groups: the same draws over the same outcome of every title.  (94, 0.9) is the
    default cell; (80, first) and (94, last) differ from their neighbours along u, so the model stage decides there."""
    import doppel_speller_amd as ds
    truth, ids, queries, actual, model, probabilities = problem
    u = 0.9 if u_index is None else probabilities[u_index]
    p = ds.Prediction(truth, ids, model, top_n=TOP_N, transform=False, levenshtein_threshold=t, probability_threshold=u)
    answer = p.generate_test_predictions(queries)["title_id"].to_numpy()
    _, out = swept
    for name, groups in (("titles", None), ("ids", actual)):
        boot = out[name][1]
        cell = boot.cell(t, u)
        expected = ds.bootstrap_accuracy([answer], actual, groups=groups, n_boot=N_BOOT, seed=SEED)
        assert boot.counts[:, cell].tobytes() == expected.counts[:, 0].tobytes(), name
        assert boot.baseline_counts[cell].tolist() == expected.baseline_counts[0].tolist()
        assert boot.n_units == expected.n_units
    if u_index is not None:
        along_u = out["titles"][1].baseline_counts.reshape(3, 4, 4)[LEVENSHTEIN.index(t)]
        assert len(np.unique(along_u, axis=0)) > 1                      # the model stage decides in this row of the grid
    if (t, u) == (94, 0.9):
        assert p.evaluate(queries, actual, n_boot=N_BOOT, groups=actual, seed=SEED) == ds.predictions_accuracy(answer, actual)
        assert p.sweep_bootstrap.counts.shape == (N_BOOT, 1, 4)
        assert p.sweep_bootstrap.counts[:, 0].tobytes() == out["ids"][1].counts[:, out["ids"][1].cell(94, 0.9)].tobytes()
        assert p.evaluate(queries, actual) == ds.predictions_accuracy(answer, actual) and p.sweep_bootstrap is None


def test_chunks_give_the_same_arrays(problem, swept):
    truth, ids, queries, actual, model, probabilities = problem
    p, out = swept
    p.chunk_queries = 7
    try:
        frame = p.threshold_sweep(queries, actual, LEVENSHTEIN, probabilities, n_boot=N_BOOT, groups=actual, seed=SEED)
    finally:
        p.chunk_queries = None
    assert _same_frame(frame, out["ids"][0])
    assert p.sweep_bootstrap.counts.tobytes() == out["ids"][1].counts.tobytes()
    assert p.sweep_bootstrap.baseline_counts.tobytes() == out["ids"][1].baseline_counts.tobytes()
    empty = p.threshold_sweep([], [], LEVENSHTEIN, probabilities, n_boot=3)
    assert len(empty) == 12 and not p.sweep_bootstrap.counts.any() and p.sweep_bootstrap.counts.shape == (3, 12, 4)
