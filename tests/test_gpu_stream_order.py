"""The stream contract of include/doppel_amd.h on a NON-BLOCKING stream: every entry point of tests/stream_cases.py's table
runs behind pending work (a gate), on inputs that exist only in stream order (a decoy is overwritten behind the gate), into
poisoned outputs, first on fresh handles (any lazy build happens in this call, on this stream, behind the gate) and then
a second time on the same handles.

  all classes   the gate's event is not ready immediately before the call ("gate too short" otherwise, never a silent
                pass); after the call's documented completion (S: on return; E, M, F: after ds_stream_sync of the test's
                stream) the outputs equal the CPU oracle of the REAL input -- bit for bit, or with the tolerance of the
                oracle's own GPU test --, equal a null-stream run of the same call, differ from the decoy's answer, and
                no byte outside what the call defines has lost its poison;
  E (F: later)  the gate's event is still not ready immediately after the call: it only enqueued;
  E, M, F       a ds_memcpy_d2d_async of every output, enqueued on the same stream with no host synchronisation after
                the call, holds the same bytes once that stream alone is synchronised.

In a row's first call a second, longer gate on the null stream delays whatever strays there until the caller's stream has
consumed its result; in its second call the null stream is idle, so a wait for it in place of the caller's stream ends at once.
"""
import time

import numpy as np
import pytest

import stream_cases as sc

pytestmark = pytest.mark.gpu

REPORT = []          # (entry, turn, class, host milliseconds of the call), printed by the last test


@pytest.fixture(autouse=True)
def stop_at_a_device_error():
    """A failure here is wrong data.  Should the device itself report an error after a test, nothing more of this module
    runs on it: the session ends there."""
    yield
    from doppel_speller_amd import _lib
    if _lib.lib().ds_stream_sync(None, 0) != 0:
        pytest.exit(f"the device reports an error after a stream-order test: {_lib.lib().ds_last_error()}", returncode=3)


@pytest.mark.parametrize("entry", [name for name, _, _ in sc.CONTRACT if name in sc.CASES])
def test_entry_point_keeps_its_stream_contract(entry, oracle):
    started = time.perf_counter()
    sc.check_contract(sc.CASES[entry](oracle), report=REPORT)
    print(f"{entry}: {time.perf_counter() - started:.2f} s")


# ---- the chain: every stage of a CandidatePipeline on the non-blocking stream ---------------------------------------------

def _snapshot(source, count, stream):
    """The first `count` elements of a device array copied on `stream`: what the stage left, before a later stage of the
    chain overwrites it."""
    from doppel_speller_amd import _lib
    kept = _lib.DeviceArray((max(count, 1),) + tuple(source.shape[1:]), source.dtype)
    size = count * int(np.prod(source.shape[1:], dtype=np.int64)) * source.dtype.itemsize
    _lib.check(_lib.lib().ds_memcpy_d2d_async(kept.ptr, source.ptr, size, 0, stream), "ds_memcpy_d2d_async")
    return kept


def _run_chain(side, table, model, k, n_rank, chunks, stream):
    """top-k, close matches, exact matches, remaining pairs, features of the remaining pairs, predict, select, then features
    and predictions of all pairs, rank, close parts and explain, chunk by chunk through ONE pipeline.  The only host
    synchronisation between stages is the one remaining_counts documents (and the gather's inside enqueue_explain)."""
    import doppel_speller_amd as ds
    ptr = None if stream is None else stream.ptr
    pipeline = ds.CandidatePipeline.over(side.index, side.table, table, k, max(last - first for first, last in chunks))
    results = []
    for first, last in chunks:
        gate = None
        if stream is not None:
            gate = sc.Gate()
            gate.close(stream)
        try:
            pipeline.load_queries_device(side.space, first, last, ptr)
            assert gate is None or gate.pending(), "gate too short: its event was ready before the first stage"
            pipeline.enqueue_top_k(ptr)
            pipeline.enqueue_close_matches(ptr)
            pipeline.enqueue_exact_matches(ptr)
            pipeline.enqueue_remaining_pairs(ptr)
            n_remaining, n_pairs = pipeline.remaining_counts(ptr)
            assert 0 < n_remaining < last - first
            pipeline.enqueue_features_remaining(n_pairs, ptr)
            pipeline.enqueue_predict(model, ptr, n_pairs)
            pipeline.enqueue_select_matches(n_remaining, stream=ptr)
            kept = [_snapshot(pipeline.d_features, n_pairs, ptr), _snapshot(pipeline._predictions, n_pairs, ptr)]
            pipeline.enqueue_features(ptr)
            pipeline.enqueue_predict(model, ptr)
            pipeline.enqueue_rank_matches(n_rank, ptr)
            pipeline.enqueue_close_parts(0, 100, ptr)
            pipeline.enqueue_explain(model, stream=ptr)
            pipeline.sync(ptr)                       # waits for that stream and reports the top-k's errors
            stages = dict(rows=pipeline.rows(), exact=pipeline.exact_matches(), counts=np.array([n_remaining, n_pairs]),
                          features_remaining=kept[0].to_host(n_pairs), predictions_remaining=kept[1].to_host(n_pairs),
                          features=pipeline.features(), predictions=pipeline.predictions())
            stages.update(zip(("ratios", "best"), pipeline.close_matches()))
            stages.update(zip(("pair_q", "pair_t"), pipeline.remaining_pairs(n_pairs)))
            stages.update(zip(("match_query", "match_row"), pipeline.matches(n_remaining)))
            stages.update(zip(("rank_row", "rank_probability", "rank_ratio", "rank_stage"), pipeline.ranked(n_rank)))
            stages.update(zip(("part_d", "part_r", "part_s"), pipeline.close_parts()))
            stages.update(zip(("explain_row", "explain_probability", "explain_count", "explain_margin",
                               "explain_features", "explain_contributions"), pipeline.explained()))
            results.append(stages)
        finally:
            if stream is not None:
                stream.sync()
                sc.sync_null()
                gate.destroy()
    return results


def test_the_whole_chain_on_a_non_blocking_stream_equals_the_null_stream():
    """A small CandidatePipeline built with `over`, its queries derived by load_queries_device, two chunks of different
    sizes (the larger first, so the second meets the first one's buffers).  The stream's run comes FIRST on fresh handles:
    the exact-match table, the truth records and the TreeSHAP paths are built by it, on the stream, behind the gate.  Every
    stage's output equals the twin pipeline's on the null stream, bit for bit."""
    import doppel_speller_amd as ds
    from doppel_speller_amd import prediction, synth
    from doppel_speller_amd.feature_engineering import encode_collection
    w = synth.make_workload(13000, 300, seed=5)
    side = prediction.TruthSide(synth._to_strings(w.t_flat, w.t_off))
    assert side.index.info()["tiles"] >= 2, "the truth set must span two score tiles"
    enc, lengths = encode_collection(*prediction._pack(synth._to_strings(w.q_flat, w.q_off)), prediction._CODE_OF)
    table = ds.TitleTable(enc, lengths)
    f = synth.make_forest(n_trees=40)
    model = ds.ForestModel(f["feature"], f["threshold"], f["yes"], f["no"], f["missing"], f["tree_offsets"], f["n_features"],
                           f["base_margin"])
    model.set_cover(np.full(model.n_nodes, 1.0) * sc._leaves_below(model.arrays))
    k, n_rank, chunks = 10, 3, ((0, 190), (190, 300))
    stream = sc.Stream()
    try:
        on_stream = _run_chain(side, table, model, k, n_rank, chunks, stream)
    finally:
        stream.close()
    on_null = _run_chain(side, table, model, k, n_rank, chunks, None)
    for chunk, (mine, twin) in enumerate(zip(on_stream, on_null)):
        assert sorted(mine) == sorted(twin)
        for name in twin:
            assert mine[name].shape == twin[name].shape and mine[name].tobytes() == twin[name].tobytes(), (chunk, name)
    stages = on_null[0]["rank_stage"]
    assert (stages == 3).any() and (stages[:, 0] == 2).any()       # model slots, and close matches at the head


# ---- the Python wrappers with a stream= parameter --------------------------------------------------------------------------------

def _flat(result):
    """The arrays of a wrapper's result, as bytes."""
    if isinstance(result, (tuple, list)):
        return tuple(part for item in result for part in _flat(item))
    return (np.ascontiguousarray(result).tobytes(),)


def _sync(stream):
    from doppel_speller_amd import _lib
    _lib.check(_lib.lib().ds_stream_sync(_lib.pointer(stream), 0), "ds_stream_sync")


def _calibrator_arrays(fitted):
    return fitted.lo, fitted.hi, fitted.pos, fitted.neg


def _wrappers():
    """{name: (inputs {name: (real, decoy)}, call(d, stream) -> arrays)}: every public function or method with a stream=
    parameter.  A call that only enqueues is followed by what its caller would do: ds_stream_sync of that stream."""
    import doppel_speller_amd as ds
    from doppel_speller_amd import _lib, bootstrap, calibration, training_set
    from doppel_speller_amd.forest import INSPECT_OVERRIDE, inspection_jobs
    from doppel_speller_amd.match_maker import TruthIndex
    from doppel_speller_amd.train import compute_cuts_device
    forest, rows = sc._forest_and_rows()
    n = rows.shape[0]
    rng = np.random.RandomState(70)
    target = (rng.rand(n) < 0.4).astype(np.float32)
    scores = rng.rand(n).astype(np.float32)
    other = sc._forest_model(dict(forest, threshold=(forest["threshold"] * np.float32(0.5)).astype(np.float32)), 66)
    model = lambda: sc._forest_model(forest, 66)()["model"]
    matrix = dict(rows=sc._pair(rows))
    labelled = dict(rows=sc._pair(rows), target=sc._pair(target))
    jobs = inspection_jobs([(0, 0, 0.0, 0), (1, 3, 0.0, 1), (INSPECT_OVERRIDE, 5, 50.0, 0)])
    x, y, small, _ = sc._training_data()
    fitted = calibration.fit_isotonic(scores, target)
    case, reverse = sc._jaccard()

    def device_out(shape, dtype, enqueue, stream):
        out = _lib.DeviceArray(shape, dtype)
        enqueue(out)
        _sync(stream)
        return out.to_host()

    def covered():
        held = model()
        held.set_cover(sc._leaves_below(forest))
        return held

    def top_k(d, stream):
        index = TruthIndex(case["rowptr"], case["truth_idx"], case["idf32"], case["sums32"])
        n_queries, k = case["q_maxint"].shape[0], case["k"]
        out = _lib.DeviceArray((n_queries, k), np.int32)
        index.top_k_device(d["q_rowptr"], d["q_cols"], d["q_maxint"], n_queries, k, out, stream)
        stats = index.sync(stream)
        return out.to_host(), index.status(n_queries, stream), np.array([stats["error_queries"]])

    def misspelled(d, stream):
        source = sc.CASES["ds_misspell_titles"](None).make()["source"]
        return training_set.misspell_table(source, np.arange(50, 250), 77, stream=stream).read()

    return {
        "ForestModel.predict_device": (matrix, lambda d, s: device_out(
            (n,), np.float32, lambda out: model().predict_device(d["rows"], n, None, out, s), s)),
        "ForestModel.count_cover_device": (matrix, lambda d, s: model().count_cover_device(d["rows"], n, stream=s)),
        "ForestModel.predict_contributions_device": (matrix, lambda d, s: device_out(
            (n, 67), np.float64, lambda out: covered().predict_contributions_device(d["rows"], n, out, stream=s), s)),
        "ForestModel.inspect_device": (labelled, lambda d, s: model().inspect_device(d["rows"], n, d["target"], jobs, 5, 0.9, s)),
        "ForestModel.permutation_importance_device": (labelled, lambda d, s: model().permutation_importance_device(
            d["rows"], n, d["target"], n_repeats=2, seed=3, features=[0, 1, 2], stream=s).counters),
        "ForestModel.partial_dependence_device": (labelled, lambda d, s: model().partial_dependence_device(
            d["rows"], n, 0, [10.0, 50.0, np.nan], d["target"], stream=s).counters),
        "ForestModel.refresh_device": (dict(rows=sc._pair(x)), lambda d, s: (lambda r: (r.node_sums, r.margins))(
            sc._forest_model(small, 6)()["model"].refresh_device(d["rows"], x.shape[0], y, stream=s))),
        "ForestModel.calibrate_device": (labelled, lambda d, s: _calibrator_arrays(
            model().calibrate_device(d["rows"], n, d["target"], s))),
        "Calibrator.transform_device": (dict(scores=sc._pair(scores)), lambda d, s: device_out(
            (n,), np.float32, lambda out: fitted.transform_device(d["scores"], n, out, s), s)),
        "calibration.fit_isotonic_device": (dict(scores=sc._pair(scores), target=sc._pair(target)), lambda d, s:
                                            _calibrator_arrays(calibration.fit_isotonic_device(d["scores"], n, d["target"], stream=s))),
        "calibration.reliability_device": (dict(scores=sc._pair(scores), target=sc._pair(target)), lambda d, s:
                                           calibration.reliability_device(d["scores"], n, d["target"], 10, stream=s).counts),
        "calibration.calibrate_rows_device": (labelled, lambda d, s: (lambda r: _calibrator_arrays(r[0]) + (r[1].counts, r[2].counts))(
            calibration.calibrate_rows_device(model(), d["rows"], n, d["target"], 10, s))),
        "bootstrap.compare_models_device": (labelled, lambda d, s: (lambda r: (r.counts, r.baseline_counts))(
            bootstrap.compare_models_device([model(), other()["model"]], d["rows"], n, d["target"], n_boot=50, seed=1, stream=s))),
        "training_set.misspell_table": ({}, misspelled),
        "TruthIndex.top_k_device, sync and status": (
            {name: sc._pair(case[name], reverse[name]) for name in ("q_rowptr", "q_cols", "q_maxint")}, top_k),
        "train.compute_cuts_device": (dict(rows=sc._pair(x)), lambda d, s: compute_cuts_device(d["rows"], x.shape[0], 256, stream=s)),
    }


WRAPPERS = ("ForestModel.predict_device", "ForestModel.count_cover_device", "ForestModel.predict_contributions_device",
            "ForestModel.inspect_device", "ForestModel.permutation_importance_device",
            "ForestModel.partial_dependence_device", "ForestModel.refresh_device", "ForestModel.calibrate_device",
            "Calibrator.transform_device", "calibration.fit_isotonic_device", "calibration.reliability_device",
            "calibration.calibrate_rows_device", "bootstrap.compare_models_device", "training_set.misspell_table",
            "TruthIndex.top_k_device, sync and status", "train.compute_cuts_device")


@pytest.mark.parametrize("name", WRAPPERS)
def test_python_wrapper_waits_for_its_own_stream(name):
    """The wrapper on the non-blocking stream, behind the gates, its device inputs staged: what it returns equals what
    it returns on the null stream for the real inputs, and is not the decoy's answer.  A wrapper that returns host data
    must have waited for THAT stream; one that frees a temporary array must not free it under pending work (the bytes
    would be another allocation's by the time the kernel runs)."""
    from doppel_speller_amd import _lib
    inputs, call = _wrappers()[name]
    upload = lambda which: {key: _lib.DeviceArray.from_host(pair[which]) for key, pair in inputs.items()}
    plain = _flat(call(upload(0), None))
    if inputs:
        assert _flat(call(upload(1), None)) != plain, "the decoy's answer equals the real one"
    for null_gate in (True, False):          # strayed work comes late next to the null-stream gate; a wait for the null
        staged, real = upload(1), upload(0)  # stream in place of the caller's ends at once when the null stream is idle
        stream, gate = sc.Stream(), sc.Gate()
        try:
            sc.sync_null()
            gate.close(stream, null_gate)
            for key in inputs:
                _lib.check(_lib.lib().ds_memcpy_d2d_async(staged[key].ptr, real[key].ptr, real[key].nbytes, 0, stream.ptr),
                           "ds_memcpy_d2d_async")
            assert gate.pending(), "gate too short: its event was ready before the call"
            got = _flat(call(staged, stream.ptr))
            assert got == plain, ("next to the null-stream gate" if null_gate else "with the null stream idle")
        finally:
            stream.close()
            sc.sync_null()
            gate.destroy()


def test_the_wrapper_list_is_complete():
    """Every public function or method of the package's modules with a `stream` parameter is in WRAPPERS (the pipeline's
    enqueue methods are the chain's, above)."""
    import inspect
    from doppel_speller_amd import bootstrap, calibration, forest, match_maker, train, training_set
    found = set()
    for module in (bootstrap, calibration, forest, match_maker, train, training_set):
        for owner in [module] + [c for _, c in inspect.getmembers(module, inspect.isclass) if c.__module__ == module.__name__]:
            for label, function in inspect.getmembers(owner, inspect.isfunction):
                if not label.startswith("_") and "stream" in inspect.signature(function).parameters and \
                        function.__module__ == module.__name__:
                    found.add(label)
    listed = {"predict_device", "count_cover_device", "predict_contributions_device", "inspect_device",
              "permutation_importance_device", "partial_dependence_device", "refresh_device", "calibrate_device",
              "transform_device", "fit_isotonic_device", "reliability_device", "calibrate_rows_device",
              "compare_models_device", "misspell_table", "top_k_device", "sync", "status", "compute_cuts_device"}
    assert found == listed, (sorted(found - listed), sorted(listed - found))


def test_the_gate_outlasts_the_slowest_enqueue():
    """Prints what tests/stream_cases.py's docstring records: the gate alone, by ds_timer, and the host time of every call
    above.  Asserts the condition only: the gate is still pending after as much host time as the slowest enqueue took."""
    from doppel_speller_amd import _lib
    stream, gate, timer = sc.Stream(), sc.Gate(), _lib.Timer()
    try:
        timer.start(stream.ptr)
        began = time.perf_counter()
        gate.close(stream, null_gate=False)
        enqueued_ms = (time.perf_counter() - began) * 1e3
        timer.stop(stream.ptr)
        assert gate.pending(), "gate too short: its event was ready as soon as it was enqueued"
        alone_ms = timer.elapsed_ms()
        enqueues = [(ms, entry, turn) for entry, turn, cls, ms in REPORT
                    if cls == sc.E or (cls == sc.F and turn == "steady state")]
        slowest = max(enqueues) if enqueues else (0.0, "-", "-")
        print(f"gate of {sc.GATE_COPIES} copies of {sc.GATE_BYTES >> 20} MiB alone: {alone_ms:.2f} ms "
              f"(enqueued in {enqueued_ms:.2f} ms of host time)")
        print(f"slowest enqueue-only call: {slowest[0]:.3f} ms ({slowest[1]}, {slowest[2]})")
        for entry, turn, cls, ms in REPORT:
            print(f"  {cls} {entry:42s} {turn:13s} {ms:9.3f} ms")
        # the same gate, with the null-stream gate next to it as in the tests, against that much host time
        gate.close(stream, null_gate=True)
        began = time.perf_counter()
        while (time.perf_counter() - began) * 1e3 < slowest[0]:
            pass
        assert gate.pending(), "gate too short: the slowest enqueue-only call outlasts it"
    finally:
        stream.close()
        sc.sync_null()
        gate.destroy()
