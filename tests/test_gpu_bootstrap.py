"""The paired bootstrap on the GPU ("Is a difference real: the paired bootstrap";
csrc/ds_bootstrap.hip) against the NumPy restatement of the rule (tests/bootstrap_oracle.py).  Everything is integers,
so everything is compared bit for bit: the counts of every case through the C ABI in its device and host forms and
through Python, under every launch option, prefixes of the replicates, the outcome codes against ds_forest_inspect,
compare_models against the oracle fed with predict's margins, train_model's bootstrap, and the library's refusals."""
import contextlib

import numpy as np
import pytest

import bootstrap_oracle as oracle

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def options(**values):
    """ds_bootstrap_option for the duration of a block; every option is back at its default afterwards."""
    from doppel_speller_amd import _lib
    defaults = dict(max_blocks=0, replicates_per_block=0, table_in_lds=1)
    try:
        for name, value in values.items():
            _lib.check(_lib.lib().ds_bootstrap_option(name.encode(), value), "ds_bootstrap_option")
        yield
    finally:
        for name in values:
            _lib.lib().ds_bootstrap_option(name.encode(), defaults[name])


def device_counts(c, n_boot=None, seed=None, fill=0):
    """ds_bootstrap_counts_device on the case's arrays -> (status, counts, baseline); the outputs start as `fill`."""
    from doppel_speller_amd import _lib
    n_boot = c["n_boot"] if n_boot is None else n_boot
    d_codes = _lib.DeviceArray.from_host(c["codes"])
    d_unit = None if c["unit"] is None else _lib.DeviceArray.from_host(c["unit"])
    d_counts = _lib.DeviceArray.from_host(np.full((n_boot, c["n_sets"], 4), fill, np.int64))
    d_baseline = _lib.DeviceArray.from_host(np.full((c["n_sets"], 4), fill, np.int64))
    try:
        status = _lib.lib().ds_bootstrap_counts_device(d_codes.ptr, c["n_sets"], c["n"], _lib.pointer(d_unit), c["n_units"],
                                                       n_boot, c["seed"] if seed is None else seed, d_counts.ptr,
                                                       d_baseline.ptr, None)
        return status, d_counts.to_host(), d_baseline.to_host()
    finally:
        for array in (d_codes, d_unit, d_counts, d_baseline):
            if array is not None:
                array.free()


def host_counts(c):
    from doppel_speller_amd import _lib
    counts = np.full((c["n_boot"], c["n_sets"], 4), -1, np.int64)
    baseline = np.full((c["n_sets"], 4), -1, np.int64)
    status = _lib.lib().ds_bootstrap_counts(_lib.pointer(c["codes"]), c["n_sets"], c["n"], _lib.pointer(c["unit"]),
                                            c["n_units"], c["n_boot"], c["seed"], _lib.pointer(counts),
                                            _lib.pointer(baseline))
    return status, counts, baseline


def same(got, c, form):
    status, counts, baseline = got
    assert status == 0, form
    assert counts.dtype == np.int64 and counts.tobytes() == c["counts"].tobytes(), (form, c["name"])
    assert baseline.tobytes() == c["baseline"].tobytes(), (form, c["name"])


# ---- 1. every case, device form and host form, under every launch option ---------------------------------------------------
@pytest.mark.parametrize("name", oracle.NAMES)
def test_counts_equal_the_oracle_in_every_form(name):
    """Covers the partial-counter widths.  Without units a lane's four class counters are 16-bit fields of one uint64
    and a wave sums them over a chunk of 2^14 draws: rows_chunks draws 70,001 times the same class, more than 16 bits
    hold, and rows_two_chunks crosses a chunk with the table in LDS.  With units the table's entries are uint32 and a
    lane's partials uint64, which no input within the limits can fill (at most 2^31 draws of entries below 2^32 is
    2^63): units_overflow, two units of 1 and 70,001 rows with every code 1, passes 2^16 in one entry and 2^17 in a
    replicate, and runs under max_blocks = 1 like every case."""
    c = oracle.case(name)
    same(device_counts(c, fill=-7), c, "device")
    same(host_counts(c), c, "host")
    for form in (dict(max_blocks=1), dict(max_blocks=3), dict(replicates_per_block=1), dict(replicates_per_block=7),
                 dict(table_in_lds=0), dict(table_in_lds=0, max_blocks=1, replicates_per_block=c["n_boot"] + 5)):
        with options(**form):
            same(device_counts(c), c, form)


@pytest.mark.parametrize("name", ["rows_257", "units_257", "units_one_holds_all", "rows_b1"])
def test_python_form_equals_the_oracle(name):
    import doppel_speller_amd as ds
    c = oracle.case(name)
    got = ds.bootstrap_counts(c["codes"], c["unit"], n_boot=c["n_boot"], seed=c["seed"])
    if c["unit"] is None:
        expected, baseline, n_units = c["counts"], c["baseline"], c["n"]
    else:                                                 # Python numbers the groups by first appearance
        unit, n_units = oracle.dense_units(c["unit"])
        expected, baseline = oracle.counts(c["codes"], unit, n_units, c["n_boot"], c["seed"])
        assert n_units == np.count_nonzero(oracle.unit_sizes(c))
        labels = np.array(["title %d" % u for u in c["unit"]])
        again = ds.bootstrap_counts(c["codes"], labels, n_boot=c["n_boot"], seed=c["seed"])
        assert again.counts.tobytes() == expected.tobytes()
    assert got.counts.tobytes() == expected.tobytes() and got.baseline.tobytes() == baseline.tobytes()
    assert got.n_units == n_units and got.seed == c["seed"]


def test_no_rows():
    import doppel_speller_amd as ds
    from doppel_speller_amd import _lib
    got = ds.bootstrap_counts(np.zeros((2, 0), np.int64), n_boot=3)
    assert got.counts.shape == (3, 2, 4) and not got.counts.any() and not got.baseline.any()
    d_counts = _lib.DeviceArray.from_host(np.full((3, 2, 4), 9, np.int64))
    d_baseline = _lib.DeviceArray.from_host(np.full((2, 4), 9, np.int64))
    assert _lib.lib().ds_bootstrap_counts_device(None, 2, 0, None, 0, 3, 1, d_counts.ptr, d_baseline.ptr, None) == 0
    assert not d_counts.to_host().any() and not d_baseline.to_host().any()
    d_counts.free()
    d_baseline.free()


# ---- 2. seeds and prefixes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rows_65", "units_256"])
def test_prefix_of_the_replicates_and_seeds(name):
    c = oracle.case(name)
    for fewer in (1, c["n_boot"] - 1):
        status, counts, baseline = device_counts(c, n_boot=fewer)
        assert status == 0 and counts.tobytes() == c["counts"][:fewer].tobytes()
        assert baseline.tobytes() == c["baseline"].tobytes()
    other = (c["seed"] + 1) & ((1 << 63) - 1)
    status, counts, baseline = device_counts(c, seed=other)
    expected, _ = oracle.counts(c["codes"], c["unit"], c["n_units"], c["n_boot"], other)
    assert status == 0 and counts.tobytes() == expected.tobytes() and counts.tobytes() != c["counts"].tobytes()
    assert baseline.tobytes() == c["baseline"].tobytes()


# ---- 3. the outcome codes ------------------------------------------------------------------------------------------------------
def lookup_forest(margins):
    """One tree that gives row i (feature 0 = i + 0.5) the margin margins[i]: a chain of splits on feature 0."""
    k = margins.shape[0]
    size = 2 * k - 1
    feature, threshold = np.full(size, -1, np.int32), np.zeros(size, np.float32)
    yes, no = np.zeros(size, np.int32), np.zeros(size, np.int32)
    for i in range(k - 1):
        feature[2 * i], threshold[2 * i], yes[2 * i], no[2 * i] = 0, i + 1, 2 * i + 1, 2 * i + 2
        threshold[2 * i + 1] = margins[i]
    threshold[size - 1] = margins[k - 1]
    return dict(feature=feature, threshold=threshold, yes=yes, no=no, missing=no.copy(),
                tree_offsets=np.array([0, size], np.int64))


def test_outcome_codes_follow_the_inspection_rule():
    import doppel_speller_amd as ds
    from doppel_speller_amd import _lib
    from doppel_speller_amd.forest import inspection_jobs
    from value_cases import neighbours
    threshold = 0.9
    cut = np.float32(np.log(threshold / (1 - threshold)))              # the margin whose probability is the threshold
    near = np.array([cut], np.float32)                                 # the cut and sixteen float32 steps either side: a
    for _ in range(16):                                                # step of the margin moves p by a third of its own
        near = np.unique(neighbours(near))
    assert near.shape[0] == 33 and near[16] == cut
    margins = np.concatenate([near, [np.nan, np.inf, -np.inf, 0.0, 1e-45, 10.0, -10.0, 88.0, -104.0]]).astype(np.float32)
    margins = np.concatenate([margins, margins])                       # every margin with both labels
    n = margins.shape[0]
    target = np.repeat([0.0, 1.0], n // 2).astype(np.float32)
    forest = lookup_forest(margins)
    model = ds.ForestModel(forest["feature"], forest["threshold"], forest["yes"], forest["no"], forest["missing"],
                           forest["tree_offsets"], 1, 0.0)
    rows = (np.arange(n, dtype=np.float32) + np.float32(0.5)).reshape(-1, 1)
    assert model.predict(rows, output_margin=True).tobytes() == margins.tobytes()
    d_margins, d_target = _lib.DeviceArray.from_host(margins), _lib.DeviceArray.from_host(target)
    d_codes = _lib.DeviceArray.from_host(np.full(n, 9, np.uint8))
    _lib.check(_lib.lib().ds_outcome_codes_device(d_margins.ptr, d_target.ptr, n, threshold, d_codes.ptr, None), "codes")
    _lib.check(_lib.lib().ds_stream_sync(None, 0), "sync")
    codes = d_codes.to_host()
    baseline = inspection_jobs([(0, 0, 0.0, 0)])
    for i in range(n):                                                 # tp, tn, fp, fn of the row on its own
        tp, tn, fp, fn = (int(v) for v in model.inspect(rows[i:i + 1], target[i:i + 1], baseline, 0, threshold)[0, :4])
        assert (tp, tn, fp, fn) == tuple(int(codes[i] == c) for c in (3, 0, 1, 2)), (i, margins[i], codes[i])
    whole = model.inspect(rows, target, baseline, 0, threshold)[0, :4]
    assert np.bincount(codes, minlength=4)[[3, 0, 1, 2]].tolist() == whole.tolist()
    nan = np.flatnonzero(np.isnan(margins))
    assert codes[nan].tolist() == [0, 2]                               # a NaN margin is not positive
    assert set(codes[:n // 2][:near.shape[0]].tolist()) == {0, 1}      # the neighbours of the cut fall on both sides
    far = np.flatnonzero(~np.isnan(margins) & (np.abs(margins - cut) > 1))
    assert codes[far].tolist() == oracle.model_codes(margins[far], target[far], threshold).tolist()
    for array in (d_margins, d_target, d_codes):
        array.free()
    model.close()


# ---- 4. compare_models -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trained():
    import doppel_speller_amd as ds
    from forest_train_oracle import make_data
    x, y = make_data(300, 12, 51)
    ex, ey = make_data(301, 12, 52)
    first = ds.ForestTrainer().fit(x, y, ex, ey, num_boost_round=4, early_stopping_rounds=4, max_depth=3, eta=0.3)
    second = ds.ForestTrainer().fit(x, y, ex, ey, num_boost_round=4, early_stopping_rounds=4, max_depth=2, eta=0.5)
    groups = np.random.RandomState(3).randint(0, 40, ex.shape[0])
    yield first, second, ex, ey, groups
    first.close()
    second.close()


def test_compare_models_equals_the_oracle(trained):
    import doppel_speller_amd as ds
    from doppel_speller_amd import _lib
    first, second, rows, target, groups = trained
    margins = [model.predict(rows, output_margin=True) for model in (first, second)]
    # between the two halves of the first model's probabilities, so that every outcome occurs
    threshold, beta = float(np.clip(np.round(np.median(first.predict(rows)), 2), 0.05, 0.95)), 3.0
    assert min(oracle.probability_gap(m, threshold) for m in margins) > 1e-6
    codes = np.stack([oracle.model_codes(m, target, threshold) for m in margins])
    assert len(np.unique(codes)) == 4 and not np.array_equal(codes[0], codes[1])
    d_rows, d_target = _lib.DeviceArray.from_host(rows), _lib.DeviceArray.from_host(target.astype(np.float32))
    for given in (None, groups):
        unit, n_units = (None, rows.shape[0]) if given is None else oracle.dense_units(given)
        expected, baseline = oracle.counts(codes, unit, n_units, 50, 17)
        got = ds.compare_models([first, second], rows, target, groups=given, n_boot=50, seed=17, threshold=threshold,
                                beta=beta, names=("deep", "shallow"))
        assert got.counts.tobytes() == expected.tobytes() and got.baseline_counts.tobytes() == baseline.tobytes()
        assert got.n_units == n_units and got.names == ("deep", "shallow") and got.weight == beta
        assert got.errors.tobytes() == oracle.errors(expected, beta).tobytes()
        assert got.baseline_errors.tolist() == oracle.errors(baseline, beta).tolist()
        for m, model in enumerate((first, second)):
            tp, tn, fp, fn = ds.evaluation_error_matrix(model, rows, target, threshold)
            assert got.baseline_counts[m].tolist() == [tn, fp, fn, tp]
        d = got.difference("deep", "shallow")
        wanted = oracle.difference(oracle.errors(expected, beta), 0, 1)
        assert d.mean == wanted["mean"] and d.interval == wanted["interval"] and d.share_better == wanted["share_better"]
        in_hbm = ds.compare_models_device([first, second], d_rows, rows.shape[0], d_target, groups=given, n_boot=50,
                                          seed=17, threshold=threshold, beta=beta)
        assert in_hbm.counts.tobytes() == got.counts.tobytes() and in_hbm.names == ("set0", "set1")
        assert in_hbm.baseline_counts.tobytes() == got.baseline_counts.tobytes()
    itself = ds.compare_models([first, first], rows, target, groups=groups, n_boot=20, threshold=threshold)
    d = itself.difference(0, 1)
    assert not d.differences.any() and d.share_better == 0.5 and d.interval == (0.0, 0.0) and d.baseline == 0
    one = ds.compare_models([second], rows, target, groups=groups, n_boot=50, seed=17, threshold=threshold, beta=beta)
    assert one.counts[:, 0].tobytes() == got.counts[:, 1].tobytes()
    d_rows.free()
    d_target.free()


def test_bootstrap_accuracy_equals_predictions_accuracy():
    import doppel_speller_amd as ds
    rng = np.random.RandomState(8)
    actual = np.where(rng.rand(500) < 0.6, rng.randint(0, 1000, 500), -1)
    sets = {}
    for name, wrong in (("strict", 0.3), ("loose", 0.1)):
        guess = np.where(rng.rand(500) < wrong, rng.randint(0, 1000, 500), actual)
        sets[name] = np.where(rng.rand(500) < 0.1, -1, guess)
    groups = rng.randint(0, 70, 500)
    got = ds.bootstrap_accuracy(sets, actual, groups=groups, n_boot=40, seed=2)
    codes = np.stack([oracle.accuracy_codes(ids, actual) for ids in sets.values()])
    unit, n_units = oracle.dense_units(groups)
    expected, baseline = oracle.counts(codes, unit, n_units, 40, 2)
    assert got.counts.tobytes() == expected.tobytes() and got.names == ("strict", "loose") and got.weight == 5.0
    for m, ids in enumerate(sets.values()):
        report = ds.predictions_accuracy(ids, actual)
        assert dict(zip(got.codes, got.baseline_counts[m].tolist())) == {k: report[k] for k in got.codes}
        assert got.baseline_errors[m] == report["custom_error"]
    assert got.difference("loose", "strict").share_better > 0.9
    listed = ds.bootstrap_accuracy(list(sets.values()), actual, groups=groups, n_boot=40, seed=2)
    assert listed.counts.tobytes() == got.counts.tobytes() and listed.names == ("set0", "set1")


# ---- 5. train_model ----------------------------------------------------------------------------------------------------------------
class _Recorder:
    """The library with the name of every entry called through it written down."""

    def __init__(self, library):
        self._library, self.calls = library, []

    def __getattr__(self, name):
        entry = getattr(self._library, name)
        if not callable(entry):
            return entry

        def call(*arguments):
            self.calls.append(name)
            return entry(*arguments)
        return call


def test_train_model_bootstrap(monkeypatch):
    """300 truth titles, 56 train titles, top_n = 20."""
    import doppel_speller_amd as ds
    from doppel_speller_amd import _lib, synth
    from doppel_speller_amd.tuning import row_groups
    w = synth.make_workload(300, 56, seed=31, query_seed=32)
    truth, train = synth._to_strings(w.t_flat, w.t_off), synth._to_strings(w.q_flat, w.q_off)
    ids = np.where(w.actual_row >= 0, w.title_id[np.maximum(w.actual_row, 0)], -1)
    data = dict(top_n=20, sample_n=4, seed=9, transform=False)
    fit = dict(num_boost_round=6, early_stopping_rounds=6, max_depth=3, eta=0.3)
    recorder = _Recorder(_lib.lib())
    monkeypatch.setattr(_lib, "lib", lambda: recorder)
    plain = ds.train_model(truth, w.title_id, train, ids, **data, **fit)
    plain_calls, recorder.calls = recorder.calls, []
    zero = ds.train_model(truth, w.title_id, train, ids, **data, **fit, bootstrap_repeats=0, bootstrap_seed=5)
    zero_calls, recorder.calls = recorder.calls, []
    assert zero_calls == plain_calls and not any("bootstrap" in name or "outcome" in name for name in zero_calls)
    assert zero.error_bootstrap is None and plain.error_bootstrap is None and "bootstrap" not in zero.timings
    assert zero.timings.keys() == plain.timings.keys()
    result = ds.train_model(truth, w.title_id, train, ids, **data, **fit, bootstrap_repeats=30, bootstrap_seed=5)
    extra = [name for name in recorder.calls if "bootstrap" in name or "outcome" in name]
    assert extra == ["ds_outcome_codes_device", "ds_bootstrap_counts_device"] and "bootstrap" in result.timings
    for a, b in ((zero, plain), (result, plain)):
        assert all(np.array_equal(a.model.arrays[k], b.model.arrays[k]) for k in ("feature", "threshold", "yes", "no"))
        assert a.history == b.history and a.error_matrix == b.error_matrix and a.rows.equals(b.rows)
    got = result.error_bootstrap
    tp, tn, fp, fn = result.error_matrix
    assert got.names == ("model",) and got.n_boot == 30 and got.seed == 5 and got.weight == 5.0
    assert got.baseline_counts.tolist() == [[tn, fp, fn, tp]]
    groups = row_groups(result.rows)[result.rows["evaluation"].to_numpy()]
    assert got.n_units == np.unique(groups).shape[0] < groups.shape[0]
    fe = ds.FeatureEngineering(truth, w.title_id, train, ids, **data)
    _, _, evaluation, evaluation_target = fe.generate_train_and_evaluation_data_sets()
    host = ds.compare_models([result.model], evaluation, evaluation_target, groups=groups, n_boot=30, seed=5)
    assert host.counts.tobytes() == got.counts.tobytes()
    # continued from a model: the returned model against the init model
    recorder.calls = []
    continued = ds.train_model(truth, w.title_id, train, ids, **data, **fit, init_model=plain.model, bootstrap_repeats=30,
                               bootstrap_seed=5)
    both = continued.error_bootstrap
    assert recorder.calls.count("ds_outcome_codes_device") == 2 and recorder.calls.count("ds_bootstrap_counts_device") == 1
    assert both.names == ("model", "init_model") and both.counts.shape == (30, 2, 4)
    assert both.counts[:, 1].tobytes() == got.counts[:, 0].tobytes()            # the init model is the plain model
    assert both.baseline_errors[1] == continued.initial_error
    d = both.difference("model", "init_model")
    assert d.baseline == both.baseline_errors[0] - both.baseline_errors[1] and 0.0 <= d.share_better <= 1.0


# ---- 6. the library's refusals ---------------------------------------------------------------------------------------------------
def test_library_refuses_bad_codes_and_units_and_leaves_the_output():
    from doppel_speller_amd import _lib
    library = _lib.lib()
    for name in ("rows_257", "units_257"):
        c = dict(oracle.case(name))
        codes = c["codes"].copy()
        codes[c["n_sets"] - 1, 200] = 4
        status, counts, baseline = device_counts(dict(c, codes=codes), fill=-7)
        assert status == -1 and b"1 codes are above 3" in library.ds_last_error()
        assert (counts == -7).all() and (baseline == -7).all()
        if c["unit"] is not None:
            for value in (-1, c["n_units"]):
                unit = c["unit"].copy()
                unit[[5, 300]] = value
                status, counts, baseline = device_counts(dict(c, unit=unit), fill=-7)
                assert status == -1 and b"2 units are outside [0, 257)" in library.ds_last_error()
                assert (counts == -7).all() and (baseline == -7).all()
        same(device_counts(c, fill=-7), c, "after a refusal")
    c = oracle.case("units_63")
    d_codes, d_unit = _lib.DeviceArray.from_host(c["codes"]), _lib.DeviceArray.from_host(c["unit"])
    d_counts = _lib.DeviceArray.from_host(np.full((c["n_boot"], c["n_sets"], 4), -7, np.int64))
    d_baseline = _lib.DeviceArray.from_host(np.full((c["n_sets"], 4), -7, np.int64))

    def call(codes=d_codes, n_sets=c["n_sets"], n=c["n"], unit=d_unit, n_units=c["n_units"], n_boot=c["n_boot"],
             counts=d_counts, baseline=d_baseline):
        return library.ds_bootstrap_counts_device(_lib.pointer(codes), n_sets, n, _lib.pointer(unit), n_units, n_boot, 1,
                                                  _lib.pointer(counts), _lib.pointer(baseline), None)
    for arguments in (dict(codes=None), dict(counts=None), dict(baseline=None), dict(n_sets=0), dict(n_sets=65),
                      dict(n_boot=0), dict(n_boot=65537), dict(n=-1), dict(n=(1 << 31) + 1), dict(n_units=0),
                      dict(n_units=(1 << 31) + 1), dict(unit=None)):
        assert call(**arguments) == -1, arguments
    assert (d_counts.to_host() == -7).all() and (d_baseline.to_host() == -7).all()
    assert call() == 0 and d_counts.to_host().tobytes() != c["counts"].tobytes()     # seed 1 is not the case's seed
    for array in (d_codes, d_unit, d_counts, d_baseline):
        array.free()
