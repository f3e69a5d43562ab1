"""The stream contract of the `_device` entry points (include/doppel_amd.h): the contract table, and the helpers that
put a call on a NON-BLOCKING stream behind pending work, with inputs that exist only in stream order.

With the null stream, or a stream made by hipStreamCreate (which the null stream implicitly joins), a launch, memset or
copy issued on the wrong stream is still ordered by accident.  Here:

  stream   hipStreamCreateWithFlags(hipStreamNonBlocking), bound through ctypes to the copy of the HIP runtime that
           libdoppel_amd.so has already mapped (its path is read from /proc/self/maps: no second runtime is loaded).
  gate     finite, ordinary work through the existing ABI: GATE_COPIES ds_memcpy_d2d_async of GATE_BYTES on the test's
           stream, an event recorded behind them.  Never a host callback or a spinning kernel: several entry points
           synchronise the stream or free scratch by design, and a gate the host releases would deadlock them.  A second
           gate, NULL_GATE_FACTOR times as long, is put on the null stream first in a row's first call: an operation that
           strays to the null stream then runs AFTER the caller's stream has consumed its result, not early by luck
           (the null stream and a non-blocking stream do not wait for each other).  The second call leaves the null
           stream idle: a synchronisation of the null stream in place of the caller's then returns at once.
  inputs   every input array has two device buffers: one holds a DECOY (an input the entry point accepts, with another
           answer), complete before the gate; the other holds the real input, and ds_memcpy_d2d_async on the test's stream
           copies real over decoy behind the gate.  The real input exists only in stream order.
  outputs  are filled with POISON bytes and have GUARD elements behind what the call defines.

Measured on an MI355X with ds_timer and time.perf_counter
(tests/test_gpu_stream_order.py::test_the_gate_outlasts_the_slowest_enqueue prints them):
  gate of 160 copies of 128 MiB alone ........................ 5.0 ms
  gate of 320 copies of 128 MiB alone (the size chosen) ...... 9.95 ms, enqueued in 1.1 ms of host time; about 27 ms
                                                               next to the null-stream gate, which shares the bandwidth
  host time of the slowest enqueue-only call ................. 0.15 ms (ds_remaining_pairs_device; first uses included:
                                                               ds_jaccard_topk_device 0.06 ms, ds_exact_matches_device
                                                               with its table build 0.04 ms)
The gate is sized to at least ten times that host time: 320 copies are 66 times it.  The tests assert the condition (the gate's event is not ready
before the call), never the number.
"""
import ctypes
import os
import re
import time

import numpy as np

# ---- the contract table: one row per prototype of include/doppel_amd.h with a `void *stream` parameter ------------------
# class E  enqueue only: returns without waiting for `stream`
#       S  `stream` is synchronised when the call returns: the outputs are complete
#       M  one synchronisation of `stream` in front (an input is read back and checked), the rest is enqueued
#       F  the FIRST call on a handle is M (a lazy build behind one synchronisation), every later call is E
# wording: a phrase of the comment in front of the prototype that says so (tests/test_stream_contract_cpu.py).
E, S, M, F = "E", "S", "M", "F"
CLASS_WORDING = {
    E: ("Asynchronous on `stream`", "asynchronous on `stream`", "without synchronising", "does not synchronise",
        "nqueued on `stream`"),
    S: ("synchronised before returning", "synchronised before the call returns", "synchronised at the end",
        "SYNCHRONISES `stream`", "Waits for `stream`", "after synchronising `stream`", "synchronises `stream`"),
    M: ("which synchronises `stream`; the rest is enqueued", "one synchronisation of `stream`"),
    F: ("After that a call only enqueues on `stream`", "after that a call only enqueues one kernel on `stream`"),
}
CONTRACT = (
    ("ds_jaccard_topk_device", E, "enqueues on `stream` and returns without synchronising"),
    ("ds_jaccard_sync", S, "Waits for `stream`"),
    ("ds_jaccard_status", S, "after synchronising `stream`"),
    ("ds_construct_features_indexed_device", F, "After that a call only enqueues on `stream`"),
    ("ds_close_matches_device", E, "enqueued on `stream`"),
    ("ds_remaining_pairs_device", E, "Asynchronous on `stream`"),
    ("ds_select_matches_device", E, "Asynchronous on `stream`"),
    ("ds_rank_matches_device", E, "Asynchronous on `stream`"),
    ("ds_exhaustive_fold_device", E, "Enqueued on `stream`"),
    ("ds_exhaustive_finish_device", E, "Asynchronous on `stream`"),
    ("ds_exhaustive_rank_device", S, "`stream` is synchronised at the end"),
    ("ds_close_parts_device", E, "Asynchronous on `stream`"),
    ("ds_threshold_sweep_device", M, "one synchronisation of `stream`"),
    ("ds_duplicate_begin_device", E, "Asynchronous on `stream`"),
    ("ds_duplicate_links_device", E, "Asynchronous on `stream`"),
    ("ds_duplicate_finish_device", E, "Asynchronous on `stream`"),
    ("ds_assign_edges_device", E, "Asynchronous on `stream`"),
    ("ds_assign_solve_device", S, "SYNCHRONISES `stream`"),
    ("ds_exact_matches_device", E, "enqueued on `stream`"),
    ("ds_forest_predict_device", E, "Asynchronous on `stream`"),
    ("ds_forest_cover_device", E, "Enqueued on `stream`"),
    ("ds_forest_contributions_device", F, "after that a call only enqueues one kernel on `stream`"),
    ("ds_forest_inspect_device", M, "which synchronises `stream`; the rest is enqueued"),
    ("ds_best_pairs_device", E, "Asynchronous on `stream`"),
    ("ds_feature_cuts_device", S, "Enqueued on `stream`, which is synchronised before returning"),
    ("ds_gather_rows_device", S, "Enqueued on `stream`, which is synchronised before returning"),
    ("ds_auc_device", S, "Enqueued on `stream` and synchronised before returning"),
    ("ds_weighted_logloss_device", S, "enqueued on `stream` and synchronised before returning, like ds_auc_device"),
    ("ds_trainer_seed_device", S, "enqueued on `stream`, which is synchronised before returning"),
    ("ds_trainer_batch_seed_device", S, "enqueued on `stream`, which is synchronised before returning"),
    ("ds_forest_refresh_device", S, "enqueued on `stream`, which is synchronised before returning"),
    ("ds_bootstrap_counts_device", S, "`stream` is synchronised before the call returns"),
    ("ds_outcome_codes_device", E, "Asynchronous on `stream`"),
    ("ds_isotonic_fit_device", S, "`stream` is synchronised before the call returns"),
    ("ds_calibration_apply_device", E, "Asynchronous on `stream`"),
    ("ds_reliability_device", E, "asynchronous on `stream`"),
    ("ds_misspell_titles", S, "Enqueued on `stream`, which is synchronised before returning"),
    ("ds_training_pairs_device", E, "Asynchronous on `stream`"),
    ("ds_hard_negatives_device", E, "enqueues three kernels on `stream` and does not synchronise"),
    ("ds_hard_total", S, "synchronises `stream`"),
    ("ds_prepare_titles", S, "Enqueued on `stream`, which is synchronised before returning"),
    ("ds_query_rows_device", E, "Asynchronous on `stream`"),
)
# plumbing with a stream parameter: the helpers above are built from them, they are what the tests order everything with
PLUMBING = ("ds_memcpy_d2d_async", "ds_stream_destroy", "ds_stream_sync", "ds_timer_start", "ds_timer_stop")
CLASS_OF = {name: cls for name, cls, _ in CONTRACT}

POISON = 0xA5
GUARD = 16
GATE_BYTES = 128 << 20
GATE_COPIES = 320
NULL_GATE_FACTOR = 2
MEASURED = dict(gate_ms=9.95, slowest_enqueue_ms=0.15)      # see the module docstring

HIP_SUCCESS, HIP_NOT_READY = 0, 600
HIP_STREAM_NON_BLOCKING = 1


def header_prototypes(text):
    """{name: (start of the prototype, its text)} of every function of the header with a `void *stream` parameter."""
    found = {}
    for match in re.finditer(r"^(?:int|int64_t|void) (ds_\w+)\(([^;]*?)\);", text, re.M | re.S):
        if re.search(r"void \*stream\b", match.group(2)):
            assert match.group(1) not in found
            found[match.group(1)] = (match.start(), match.group(0))
    return found


def comment_before(text, start):
    """The text of the last comment block that ends in front of position `start` (prototypes may stand between: one block
    often describes the entry points that follow it), its line breaks and their ` * ` taken out."""
    end = text.rfind("*/", 0, start)
    while end >= 0:
        begin = text.rfind("/*", 0, end)
        # a trailing remark on a prototype's own line is no description
        line_start = text.rfind("\n", 0, begin) + 1
        if text[line_start:begin].strip() == "":
            return re.sub(r"\s+", " ", re.sub(r"\n \*", " ", text[begin:end + 2]))
        end = text.rfind("*/", 0, begin)
    return ""


# ---- the HIP runtime the library has mapped --------------------------------------------------------------------------------

_hip = None


def hip():
    global _hip
    if _hip is None:
        from doppel_speller_amd import _lib
        _lib.lib()
        path = None
        with open("/proc/self/maps") as maps:
            for line in maps:
                fields = line.split()
                if len(fields) >= 6 and os.path.basename(fields[5]).startswith("libamdhip64"):
                    path = fields[5]
                    break
        assert path is not None, "libdoppel_amd.so has mapped no HIP runtime"
        runtime = ctypes.CDLL(path)           # the path that is already mapped: dlopen hands back the same object
        p = ctypes.c_void_p
        runtime.hipStreamCreateWithFlags.argtypes = [ctypes.POINTER(p), ctypes.c_uint]
        runtime.hipStreamDestroy.argtypes = [p]
        runtime.hipEventCreate.argtypes = [ctypes.POINTER(p)]
        runtime.hipEventRecord.argtypes = [p, p]
        runtime.hipEventQuery.argtypes = [p]
        runtime.hipEventDestroy.argtypes = [p]
        runtime.hipMemcpyAsync.argtypes = [p, p, ctypes.c_size_t, ctypes.c_int, p]
        _hip = runtime
    return _hip


class Stream:
    """A non-blocking stream; `ptr` goes wherever the ABI takes a stream."""

    def __init__(self):
        self.ptr = ctypes.c_void_p()
        assert hip().hipStreamCreateWithFlags(ctypes.byref(self.ptr), HIP_STREAM_NON_BLOCKING) == HIP_SUCCESS

    def sync(self):
        from doppel_speller_amd import _lib
        _lib.check(_lib.lib().ds_stream_sync(self.ptr, 0), "ds_stream_sync")

    def close(self):
        if self.ptr:
            self.sync()
            assert hip().hipStreamDestroy(self.ptr) == HIP_SUCCESS
            self.ptr = None


def read_on(reader, array):
    """A device array copied to the host on the non-blocking stream `reader`.  ds_memcpy_d2h is a hipMemcpy, which joins the
    null stream: it would wait for exactly the strayed work whose lateness the tests are there to see."""
    from doppel_speller_amd import _lib
    out = np.empty(array.shape, dtype=array.dtype)
    if out.nbytes:
        assert hip().hipMemcpyAsync(_lib.pointer(out), array.ptr, out.nbytes, 2, reader.ptr) == HIP_SUCCESS   # device to host
    reader.sync()
    return out


def sync_null():
    from doppel_speller_amd import _lib
    _lib.check(_lib.lib().ds_stream_sync(None, 0), "ds_stream_sync")


class Gate:
    """Pending work in front of a call (see the module docstring).  One per process: two pairs of buffers."""
    _buffers = None

    def __init__(self):
        from doppel_speller_amd import _lib
        if Gate._buffers is None:
            Gate._buffers = [_lib.DeviceArray((GATE_BYTES,), np.uint8) for _ in range(4)]
            for buffer in Gate._buffers:
                _lib.check(_lib.lib().ds_memset(buffer.ptr, 0, buffer.nbytes, 0), "ds_memset")
            sync_null()
        self.event = ctypes.c_void_p()
        assert hip().hipEventCreate(ctypes.byref(self.event)) == HIP_SUCCESS

    def close(self, stream, null_gate=True):
        """Puts the gate on `stream` (and the longer one on the null stream) and records the event behind it."""
        from doppel_speller_amd import _lib
        copy = _lib.lib().ds_memcpy_d2d_async
        a, b, c, d = Gate._buffers
        if null_gate:
            for _ in range(GATE_COPIES * NULL_GATE_FACTOR):
                _lib.check(copy(d.ptr, c.ptr, GATE_BYTES, 0, None), "ds_memcpy_d2d_async")
        for _ in range(GATE_COPIES):
            _lib.check(copy(b.ptr, a.ptr, GATE_BYTES, 0, stream.ptr), "ds_memcpy_d2d_async")
        assert hip().hipEventRecord(self.event, stream.ptr) == HIP_SUCCESS

    def pending(self):
        status = hip().hipEventQuery(self.event)
        assert status in (HIP_SUCCESS, HIP_NOT_READY), status
        return status == HIP_NOT_READY

    def destroy(self):
        if self.event:
            hip().hipEventDestroy(self.event)
            self.event = None


# ---- a case: one entry point, its real and decoy inputs, its outputs and its oracle -------------------------------------------

class Spec:
    """entry: the entry point.  inputs: {name: (real, decoy)} host arrays of equal shape and dtype, staged in HBM.
    outputs: {name: (dtype, elements)} device buffers the call writes; host_outputs: the same for host arrays.
    inout: inputs the call also writes (compared like outputs, no poison).  scratch: outputs whose contents are not
    defined.  make() -> the handles, created fresh.  call(lib, handles, p, stream) -> status, p[name] the pointer of every
    input and output.  expect(values) -> {name: the oracle's array}, for values = {name: host array}; an output is compared
    over the oracle's elements, bit for bit, and must be poison behind them; compare[name](whole buffer, want) -> bool
    replaces both where a part of an output is a diagnostic or has a tolerance of its oracle's GPU test.
    collect(lib, handles, p): reads what the call left behind a handle into host outputs, after the call's completion.
    expect_second: the oracle of the second call on the same handles, where calls accumulate.  once: the call is legal
    once per handle, so the second call gets fresh handles of its own."""

    def __init__(self, entry, inputs, expect, call, outputs=None, host_outputs=None, inout=(), scratch=(), make=None,
                 compare=None, label=None, collect=None, expect_second=None, once=False):
        self.entry, self.inputs, self.expect, self.call = entry, inputs, expect, call
        self.collect, self.expect_second, self.once = collect, expect_second or expect, once
        self.outputs, self.host_outputs = outputs or {}, host_outputs or {}
        self.inout, self.scratch, self.make = tuple(inout), tuple(scratch), make or (lambda: {})
        self.compare, self.label = compare or {}, label or entry
        for name, (real, decoy) in inputs.items():
            assert real.shape == decoy.shape and real.dtype == decoy.dtype, name
            assert real.flags["C_CONTIGUOUS"] and decoy.flags["C_CONTIGUOUS"], name

    def values(self, which):
        return {name: pair[which] for name, pair in self.inputs.items()}

    def oracle_answers_differ(self):
        """The decoy's answer must differ from the real one, or a call that read the decoy would pass."""
        if not self.inputs:
            return True                     # nothing staged: the row checks order, completion and poison only
        real, decoy = self.expect(self.values(0)), self.expect(self.values(1))
        return any(np.asarray(real[name]).tobytes() != np.asarray(decoy[name]).tobytes() for name in real)


def _poisoned(dtype, count):
    return np.frombuffer(bytes([POISON]) * ((count + GUARD) * np.dtype(dtype).itemsize), dtype=dtype).copy()


class Buffers:
    """The device and host buffers of one call of a Spec."""

    def __init__(self, spec, first, second=None):
        """first: what the input buffers hold now; second: what lies in the twin buffers, copied over later (or None)."""
        from doppel_speller_amd import _lib
        self.spec, lib = spec, _lib.lib()
        hold = lambda array: _lib.DeviceArray.from_host(array if array.size else np.zeros(1, array.dtype))
        self.d_in = {name: hold(array) for name, array in first.items()}
        self.d_twin = {name: hold(array) for name, array in (second or {}).items()}
        self.d_out = {name: _lib.DeviceArray((count + GUARD,), dtype) for name, (dtype, count) in spec.outputs.items()}
        for out in self.d_out.values():
            _lib.check(lib.ds_memset(out.ptr, POISON, out.nbytes, 0), "ds_memset")
        self.h_out = {name: _poisoned(dtype, count) for name, (dtype, count) in spec.host_outputs.items()}
        self.d_copy = {}
        sync_null()

    def pointers(self):
        from doppel_speller_amd import _lib
        p = {name: array.ptr for name, array in self.d_in.items()}
        p.update({name: array.ptr for name, array in self.d_out.items()})
        p.update({name: _lib.pointer(array) for name, array in self.h_out.items()})
        return p

    def release(self, stream):
        """real over decoy, in stream order."""
        from doppel_speller_amd import _lib
        for name, twin in self.d_twin.items():
            _lib.check(_lib.lib().ds_memcpy_d2d_async(self.d_in[name].ptr, twin.ptr, self.spec.inputs[name][0].nbytes, 0,
                                                      stream.ptr), "ds_memcpy_d2d_async")

    def _written(self):
        written = dict(self.d_out)
        written.update({name: self.d_in[name] for name in self.spec.inout})
        return written

    def copy_outputs(self, stream):
        """The consumer: every device output copied on `stream`, with no host synchronisation in between."""
        from doppel_speller_amd import _lib
        for name, array in self._written().items():
            twin = _lib.DeviceArray(array.shape, array.dtype)
            _lib.check(_lib.lib().ds_memcpy_d2d_async(twin.ptr, array.ptr, array.nbytes, 0, stream.ptr),
                       "ds_memcpy_d2d_async")
            self.d_copy[name] = twin

    def read(self, copies=False, reader=None):
        source = self.d_copy if copies else self._written()
        fetch = (lambda array: array.to_host()) if reader is None else (lambda array: read_on(reader, array))
        got = {name: fetch(array).reshape(-1) for name, array in source.items()}
        got.update(self.h_out)
        return got

    def free(self):
        for group in (self.d_in, self.d_twin, self.d_out, self.d_copy):
            for array in group.values():
                array.free()


def check_outputs(spec, got, want, what):
    """`got` (whole buffers) against the oracle's `want`: the defined elements, then poison to the end."""
    names = set(spec.outputs) | set(spec.host_outputs) | set(spec.inout)
    assert set(want) == names - set(spec.scratch), (what, sorted(want), sorted(names))
    for name, expected in want.items():
        expected = np.ascontiguousarray(expected).reshape(-1)
        mine = got[name].reshape(-1)
        assert mine.dtype == expected.dtype and mine.shape[0] >= expected.shape[0], (what, name, mine.dtype, expected.dtype)
        head = mine[:expected.shape[0]]
        if name in spec.compare:
            assert spec.compare[name](mine, expected), (what, name, head[:8], expected[:8])
            continue
        else:
            wrong = np.nonzero(head.view(np.uint8).reshape(expected.shape[0], -1) !=
                               expected.view(np.uint8).reshape(expected.shape[0], -1))[0] if expected.shape[0] else ()
            assert len(wrong) == 0, (what, name, len(wrong), wrong[:5], head[wrong[:5]], expected[wrong[:5]])
        if name not in spec.inout:
            assert (mine[expected.shape[0]:].view(np.uint8) == POISON).all(), (what, name, "wrote past what it defines")


def run_on_null_stream(spec, values, handles=None):
    """The plain call: inputs complete, the null stream, one synchronisation -> the outputs."""
    from doppel_speller_amd import _lib
    handles = spec.make() if handles is None else handles
    buffers = Buffers(spec, values)
    try:
        pointers = buffers.pointers()
        status = spec.call(_lib.lib(), handles, pointers, ctypes.c_void_p(0))
        assert status == 0, (spec.label, status, _lib.lib().ds_last_error())
        sync_null()
        if spec.collect is not None:
            spec.collect(_lib.lib(), handles, pointers)
        return buffers.read()
    finally:
        buffers.free()


class Staged:
    """One call on a non-blocking stream behind a gate, its inputs staged and its outputs poisoned."""

    def __init__(self, spec, handles, stream, null_gate=True):
        from doppel_speller_amd import _lib
        reader = Stream()                    # the outputs are read on a stream of their own: see read_on
        self.spec, self.cls = spec, CLASS_OF[spec.entry]
        buffers, gate = Buffers(spec, spec.values(1), spec.values(0)), Gate()
        self.copies = None
        try:
            gate.close(stream, null_gate)
            buffers.release(stream)
            self.pending_before = gate.pending()
            started = time.perf_counter()
            pointers = buffers.pointers()
            self.status = spec.call(_lib.lib(), handles, pointers, stream.ptr)
            self.host_ms = (time.perf_counter() - started) * 1e3
            self.pending_after = gate.pending()
            self.error = _lib.lib().ds_last_error() if self.status else b""
            if self.status != 0:
                self.outputs = None
            elif self.cls == S:
                if spec.collect is not None:
                    spec.collect(_lib.lib(), handles, pointers)
                self.outputs = buffers.read(reader=reader)      # complete on return: no synchronisation of the test's own
            else:
                buffers.copy_outputs(stream)
                stream.sync()                            # that stream only
                if spec.collect is not None:
                    spec.collect(_lib.lib(), handles, pointers)
                self.outputs, self.copies = buffers.read(reader=reader), buffers.read(copies=True, reader=reader)
        finally:
            stream.sync()
            sync_null()
            gate.destroy()
            buffers.free()
            reader.close()


def check_contract(spec, oracle_real=None, null_gate=True, report=None):
    """Everything the contract asks of one row: see tests/test_gpu_stream_order.py."""
    cls = CLASS_OF[spec.entry]
    assert spec.oracle_answers_differ(), (spec.label, "the decoy's answer equals the real one")
    want = spec.expect(spec.values(0)) if oracle_real is None else oracle_real
    # the decoy runs clean, the plain way, and both plain answers are the oracle's
    if spec.inputs:
        check_outputs(spec, run_on_null_stream(spec, spec.values(1)), spec.expect(spec.values(1)),
                      (spec.label, "decoy on the null stream"))
    plain = run_on_null_stream(spec, spec.values(0))
    check_outputs(spec, plain, want, (spec.label, "null stream"))
    handles, stream = spec.make(), Stream()
    try:
        for turn in ("first use", "steady state"):
            if turn == "steady state" and spec.once:
                handles = spec.make()
            # the first use runs next to the null-stream gate: a lazy build or launch that strays there comes too late.
            # The second call runs with the null stream idle: a wait for the null stream instead of the caller's then
            # returns at once (next to the longer null-stream gate it would outlast the caller's work by luck).
            run = Staged(spec, handles, stream, null_gate and turn == "first use")
            what = (spec.label, turn)
            if turn == "steady state" and spec.expect_second is not spec.expect:
                want, plain = spec.expect_second(spec.values(0)), None
            if report is not None:
                report.append((spec.label, turn, cls, run.host_ms))
            assert run.pending_before, (what, "gate too short: its event was ready before the call")
            assert run.status == 0, (what, run.status, run.error)
            for got, form in ((run.outputs, "outputs"), (run.copies, "a copy enqueued behind the call")):
                if got is None:
                    continue
                check_outputs(spec, got, want, what + (form,))
                for name in want:
                    if name not in spec.compare and plain is not None:
                        assert got[name].tobytes() == plain[name].tobytes(), what + (form, name, "differs from the null stream's")
            if cls == E or (cls == F and turn == "steady state"):
                assert run.pending_after, (what, "the call waited for the caller's earlier work: it does not only enqueue")
    finally:
        stream.close()


# ---- the cases: one per row, from the case modules and oracles the kernels' own tests use ------------------------------------
# A builder needs no GPU: handles are made by the Spec's make(), inside the test.  Decoys are zero bytes wherever that is an
# input the entry point accepts (row 0, score 0, label 0, no edge), otherwise another accepted input of the same shape.

def _pair(real, decoy=None, dtype=None):
    real = np.ascontiguousarray(real, dtype=dtype)
    decoy = np.zeros_like(real) if decoy is None else np.ascontiguousarray(decoy, dtype=real.dtype)
    return real, decoy


def _out_pointer(pointer, ctype):
    return ctypes.cast(pointer, ctypes.POINTER(ctype))


def case_rank_matches(oracle):
    import ranked_cases as rc
    n_queries, k, n, n_truth = 203, 17, 5, 36
    groups = rc.make_groups(n_queries, k, n_truth, seed=3)
    dtypes = (np.int32, np.float32, np.uint8, np.int32, np.int32)
    names = ("rows", "probabilities", "ratios", "exact", "best")
    outputs = ("out_row", "out_probability", "out_ratio", "out_stage")
    inputs = {name: _pair(array, dtype=dtype) for name, array, dtype in zip(names, groups, dtypes)}

    def expect(v):
        return dict(zip(outputs, rc.rank_matches(*(v[name] for name in names), n, n_truth)))

    def call(lib, h, p, stream):
        return lib.ds_rank_matches_device(*(p[name] for name in names), n_queries, k, n, n_truth,
                                          *(p[name] for name in outputs), stream)
    sizes = dict(zip(outputs, ((np.int32, n_queries * n), (np.float32, n_queries * n), (np.uint8, n_queries * n),
                               (np.int8, n_queries * n))))
    return Spec("ds_rank_matches_device", inputs, expect, call, outputs=sizes)


def case_assign_edges(oracle):
    import assignment_cases as ac
    case = ac.small(64, 4, 30)
    count, n = case.row.shape
    names = ("row", "probability", "ratio", "stage")
    dtypes = (np.int32, np.float32, np.uint8, np.int8)
    inputs = {name: _pair(getattr(case, name), dtype=dtype) for name, dtype in zip(names, dtypes)}

    def expect(v):
        slots = ac.Case(v["row"], v["probability"], v["ratio"], v["stage"], case.n_truth, case.threshold)
        return dict(edge_key=ac.keys_of(slots).astype(np.uint64), edge_row=v["row"])

    def call(lib, h, p, stream):
        return lib.ds_assign_edges_device(*(p[name] for name in names), 0, count, count, n, case.n_truth,
                                          float(case.threshold), p["edge_key"], p["edge_row"], stream)
    return Spec("ds_assign_edges_device", inputs, expect, call,
                outputs=dict(edge_key=(np.uint64, count * n), edge_row=(np.int32, count * n)))


def case_assign_solve(oracle):
    import assignment_cases as ac
    case = ac.random_ties(count=3000, n=5, n_truth=700, seed=17)
    count, n = case.row.shape
    inputs = dict(edge_row=_pair(case.row, dtype=np.int32), edge_key=_pair(ac.keys_of(case), dtype=np.uint64))
    per_title = ("match_row", "match_slot", "first_row")

    def expect(v):
        result = ac.deferred_acceptance(v["edge_row"], v["edge_key"], case.n_truth)
        want = {name: np.asarray(getattr(result, name), dtype=np.int32) for name in per_title}
        return dict(want, counts=np.asarray(result.counts, dtype=np.int64))

    def call(lib, h, p, stream):
        return lib.ds_assign_solve_device(p["edge_row"], p["edge_key"], count, n, case.n_truth, p["held"], p["next"],
                                          *(p[name] for name in per_title), p["counts"], stream)
    outputs = dict(held=(np.uint64, case.n_truth), next=(np.int32, count), counts=(np.int64, 6))
    outputs.update({name: (np.int32, count) for name in per_title})
    # counts[4] and [5] (proposals, rounds) depend on the schedule: diagnostics, as in the kernel's own test
    return Spec("ds_assign_solve_device", inputs, expect, call, outputs=outputs, scratch=("held", "next"),
                compare=dict(counts=lambda got, want: got[:4].tolist() == want[:4].tolist() and
                             (got[6:].view(np.uint8) == POISON).all()))


def case_remaining_pairs(oracle):
    n, k, q_first = 2500, 3, 11
    rng = np.random.RandomState(8)
    best = np.where(rng.rand(n) < 0.5, -1, rng.randint(0, 1 << 30, n)).astype(np.int32)
    rows = rng.randint(0, 1 << 30, (n, k)).astype(np.int32)
    inputs = dict(best=_pair(best), rows=_pair(rows))

    def expect(v):
        pair_q, pair_t = oracle.remaining_pairs(v["best"], v["rows"])
        remaining = int((v["best"] < 0).sum())
        return dict(pair_q=(q_first + np.asarray(pair_q)).astype(np.int32), pair_t=np.asarray(pair_t, dtype=np.int32),
                    counts=np.array([remaining, remaining * k], dtype=np.int64))

    def call(lib, h, p, stream):
        return lib.ds_remaining_pairs_device(p["best"], p["rows"], n, k, q_first, p["pair_q"], p["pair_t"], p["counts"],
                                             stream)
    blocks = (n + 1023) // 1024
    # behind the two totals the counts are scratch (the blocks' scan)
    return Spec("ds_remaining_pairs_device", inputs, expect, call,
                outputs=dict(pair_q=(np.int32, n * k), pair_t=(np.int32, n * k), counts=(np.int64, 2 + blocks)),
                compare=dict(counts=lambda got, want: got[:2].tolist() == want.tolist() and
                             (got[2 + blocks:].view(np.uint8) == POISON).all()))


def case_select_matches(oracle):
    n, k, threshold = 1029, 4, 0.9
    rng = np.random.RandomState(12)
    values = np.array([0.05, 0.3, 0.9, 0.93, 0.97, 0.99], dtype=np.float32)
    predictions = values[rng.randint(0, values.shape[0], n * k)]
    pair_q = np.repeat(rng.randint(1, 1 << 30, n).astype(np.int32), k)
    pair_t = rng.randint(1, 1 << 30, n * k).astype(np.int32)
    inputs = dict(pair_q=_pair(pair_q), pair_t=_pair(pair_t), predictions=_pair(predictions))

    def expect(v):
        query, row = oracle.select_matches(v["pair_q"], v["pair_t"], v["predictions"], k, threshold)
        return dict(match_query=np.asarray(query, dtype=np.int32), match_row=np.asarray(row, dtype=np.int32))

    def call(lib, h, p, stream):
        return lib.ds_select_matches_device(p["pair_q"], p["pair_t"], p["predictions"], n, k, threshold,
                                            p["match_query"], p["match_row"], stream)
    return Spec("ds_select_matches_device", inputs, expect, call,
                outputs=dict(match_query=(np.int32, n), match_row=(np.int32, n)))


def _slots_of_keys(keys):
    """ds_exhaustive_finish_device's rule: (row, probability) of a key, (-1, quiet NaN) of an empty one."""
    keys = np.asarray(keys, dtype=np.uint64).reshape(-1)
    empty = keys == 0
    row = (np.uint64(0xffffffff) - (keys & np.uint64(0xffffffff))).astype(np.int64)
    bits = (keys >> np.uint64(32)).astype(np.uint32)
    return (np.where(empty, -1, row).astype(np.int32),
            np.where(empty, np.uint32(0x7fc00000), bits).astype(np.uint32).view(np.float32))


def case_exhaustive_fold(oracle):
    import exhaustive_cases as ec
    n_queries, n_rows, n = 3, 300, 5
    probabilities = ec.make_probabilities(n_queries, n_rows, "few", seed=9)
    inputs = dict(probabilities=_pair(probabilities, dtype=np.float32),
                  running=_pair(np.zeros((n_queries, n), dtype=np.uint64)))

    def expect(v):
        return dict(running=np.asarray(ec.best_keys(v["probabilities"], n), dtype=np.uint64))

    def call(lib, h, p, stream):
        return lib.ds_exhaustive_fold_device(p["probabilities"], n_queries, n_rows, 0, n, p["running"], stream)
    return Spec("ds_exhaustive_fold_device", inputs, expect, call, inout=("running",))


def case_exhaustive_finish(oracle):
    import exhaustive_cases as ec
    n_queries, n = 257, 7
    keys = ec.best_keys(ec.make_probabilities(n_queries, 40, "random", seed=4), n)
    inputs = dict(running=_pair(keys, dtype=np.uint64))

    def expect(v):
        return dict(zip(("out_row", "out_probability"), _slots_of_keys(v["running"])))

    def call(lib, h, p, stream):
        return lib.ds_exhaustive_finish_device(p["running"], n_queries, n, p["out_row"], p["out_probability"], stream)
    return Spec("ds_exhaustive_finish_device", inputs, expect, call,
                outputs=dict(out_row=(np.int32, n_queries * n), out_probability=(np.float32, n_queries * n)))


def case_duplicate_begin(oracle):
    n_truth = 3001

    def expect(v):
        return dict(parent=np.arange(n_truth, dtype=np.int32), counts=np.zeros(3, dtype=np.int64))

    def call(lib, h, p, stream):
        return lib.ds_duplicate_begin_device(p["parent"], n_truth, p["counts"], stream)
    return Spec("ds_duplicate_begin_device", {}, expect, call,
                outputs=dict(parent=(np.int32, n_truth), counts=(np.int64, 3)))


def _roots(parent):
    parent = np.asarray(parent, dtype=np.int64)
    while True:
        above = parent[parent]
        if np.array_equal(above, parent):
            return parent
        parent = above


def case_duplicate_links(oracle):
    import duplicates_cases as dc
    n_truth, k = 2000, 4
    (q_first, rows, ratios, probabilities, exact), = dc.random_links(n_truth, k, seed=5)
    inputs = dict(rows=_pair(rows, dtype=np.int32), ratios=_pair(ratios, dtype=np.uint8),
                  probabilities=_pair(probabilities, dtype=np.float32), exact=_pair(exact, dtype=np.int32),
                  parent=_pair(np.arange(n_truth, dtype=np.int32), np.arange(n_truth, dtype=np.int32)),
                  counts=_pair(np.zeros(3, dtype=np.int64)))

    def expect(v):
        calls = [(q_first, v["rows"], v["ratios"], v["probabilities"], v["exact"])]
        labels, _, reasons, counts = dc.expected(calls, n_truth, dc.T, dc.U)
        return dict(parent=np.asarray(labels, dtype=np.int32), reason=np.asarray(reasons[0], dtype=np.uint8),
                    counts=np.asarray(counts, dtype=np.int64))

    def call(lib, h, p, stream):
        return lib.ds_duplicate_links_device(p["rows"], p["ratios"], p["probabilities"], p["exact"], q_first, n_truth, k,
                                             n_truth, int(dc.T), float(dc.U), p["parent"], p["reason"], p["counts"], stream)
    # before the finish only the ROOT of every row is a function of the links; the pointers below it follow the schedule
    return Spec("ds_duplicate_links_device", inputs, expect, call, outputs=dict(reason=(np.uint8, n_truth * k)),
                inout=("parent", "counts"),
                compare=dict(parent=lambda got, want: (got <= np.arange(n_truth)).all() and
                             np.array_equal(_roots(got), want)))


def case_duplicate_finish(oracle):
    n_truth = 3001
    at = np.arange(n_truth, dtype=np.int32)
    parent = np.where(at % 5 == 0, at, at - 1).astype(np.int32)          # paths of five rows: 0-1-2-3-4, 5-..

    def expect(v):
        labels = _roots(v["parent"]).astype(np.int32)
        return dict(parent=labels, label=labels, size=np.bincount(labels, minlength=n_truth)[labels].astype(np.int32))

    def call(lib, h, p, stream):
        return lib.ds_duplicate_finish_device(p["parent"], n_truth, p["label"], p["size"], stream)
    return Spec("ds_duplicate_finish_device", dict(parent=_pair(parent)), expect, call, inout=("parent",),
                outputs=dict(label=(np.int32, n_truth), size=(np.int32, n_truth)))


def case_best_pairs(oracle):
    import query_cases as qc
    n, k = 257, 7
    rows, probabilities = qc.best_pair_case(n, k, seed=1000 * k + n)
    inputs = dict(rows=_pair(rows, dtype=np.int32), probabilities=_pair(probabilities, dtype=np.float32))
    outputs = ("best_pair", "best_row", "best_probability", "best_count")

    def expect(v):
        pair, row, bits, count = qc.best_pairs_loop(v["rows"], v["probabilities"])
        return dict(zip(outputs, (np.asarray(pair, dtype=np.int64), np.asarray(row, dtype=np.int32),
                                  np.asarray(bits, dtype=np.uint32).view(np.float32), np.asarray(count, dtype=np.int32))))

    def call(lib, h, p, stream):
        return lib.ds_best_pairs_device(p["rows"], p["probabilities"], n, k, *(p[name] for name in outputs), stream)
    return Spec("ds_best_pairs_device", inputs, expect, call,
                outputs=dict(zip(outputs, ((np.int64, n), (np.int32, n), (np.float32, n), (np.int32, n)))))


def case_outcome_codes(oracle):
    import bootstrap_oracle
    n, threshold = 4099, 0.9
    rng = np.random.RandomState(6)
    margins = (rng.randint(-12, 13, n) * 0.5).astype(np.float32)          # sigmoid(k / 2) is nowhere near 0.9
    margins[::97] = np.nan
    target = (rng.rand(n) < 0.4).astype(np.float32)
    inputs = dict(margins=_pair(margins), target=_pair(target))

    def expect(v):
        return dict(codes=bootstrap_oracle.model_codes(v["margins"], v["target"], threshold).astype(np.uint8))

    def call(lib, h, p, stream):
        return lib.ds_outcome_codes_device(p["margins"], p["target"], n, threshold, p["codes"], stream)
    return Spec("ds_outcome_codes_device", inputs, expect, call, outputs=dict(codes=(np.uint8, n)))


def case_calibration_apply(oracle):
    import calibration_oracle
    n, K = 5000, 300
    rng = np.random.RandomState(21)
    lo = np.unique(rng.rand(2 * K).astype(np.float32))[:K]
    value = np.sort(rng.rand(K)).astype(np.float32)
    scores = rng.rand(n).astype(np.float32)
    scores[::50], scores[1::50] = np.nan, lo[rng.randint(0, K, n // 50)]
    # the edges stay the real ones in the decoy: K zeros are no ascending edges
    inputs = dict(lo=_pair(lo, lo), value=_pair(value), scores=_pair(scores))

    def expect(v):
        return dict(out=calibration_oracle.transform(v["lo"], v["value"], v["scores"]))

    def call(lib, h, p, stream):
        return lib.ds_calibration_apply_device(p["lo"], p["value"], K, p["scores"], n, p["out"], stream)
    return Spec("ds_calibration_apply_device", inputs, expect, call, outputs=dict(out=(np.float32, n)))


def case_reliability(oracle):
    import calibration_oracle
    n, n_bins = 6000, 10
    rng = np.random.RandomState(22)
    probabilities = rng.rand(n).astype(np.float32)
    probabilities[::40], probabilities[1::40], probabilities[2::40] = np.nan, 1.5, 1.0
    target = (rng.rand(n) < probabilities).astype(np.float32)
    inputs = dict(probabilities=_pair(probabilities), target=_pair(target))

    def expect(v):
        return dict(out=calibration_oracle.reliability(v["probabilities"], v["target"], n_bins).astype(np.int64))

    def call(lib, h, p, stream):
        return lib.ds_reliability_device(p["probabilities"], p["target"], n, n_bins, p["out"], stream)
    return Spec("ds_reliability_device", inputs, expect, call, outputs=dict(out=(np.int64, (n_bins + 1) * 4)))


def case_isotonic_fit(oracle):
    import calibration_cases
    import calibration_oracle
    # two sort tiles, the head scan and both pooling levels
    scores, target = calibration_cases.fit_cases()["alternating_8193"]
    n = scores.shape[0]
    inputs = dict(scores=_pair(scores, dtype=np.float32), target=_pair(target, dtype=np.float32))
    blocks = ("lo", "hi", "pos", "neg")

    def expect(v):
        fitted = calibration_oracle.fit(v["scores"], v["target"])
        want = {name: fitted[name] for name in blocks}
        return dict(want, out=np.array([fitted["lo"].shape[0], fitted["n_nan"], fitted["n_points"]], dtype=np.int64))

    def call(lib, h, p, stream):
        return lib.ds_isotonic_fit_device(p["scores"], p["target"], n, *(p[name] for name in blocks), p["out"], stream)
    # out[3], the blocks that entered the serial level, is a diagnostic of the segment width
    return Spec("ds_isotonic_fit_device", inputs, expect, call,
                outputs=dict(lo=(np.float32, n), hi=(np.float32, n), pos=(np.int64, n), neg=(np.int64, n)),
                host_outputs=dict(out=(np.int64, 4)),
                compare=dict(out=lambda got, want: got[:3].tolist() == want.tolist() and want[0] <= got[3] <= want[2] and
                             (got[4:].view(np.uint8) == POISON).all()))


def case_bootstrap_counts(oracle):
    import bootstrap_oracle
    c = bootstrap_oracle.case("units_257")
    inputs = dict(codes=_pair(c["codes"], dtype=np.uint8), unit=_pair(c["unit"], dtype=np.int32))

    def expect(v):
        counts, baseline = bootstrap_oracle.counts(v["codes"], v["unit"], c["n_units"], c["n_boot"], c["seed"])
        return dict(counts=np.asarray(counts, dtype=np.int64), baseline=np.asarray(baseline, dtype=np.int64))

    def call(lib, h, p, stream):
        return lib.ds_bootstrap_counts_device(p["codes"], c["n_sets"], c["n"], p["unit"], c["n_units"], c["n_boot"],
                                              c["seed"], p["counts"], p["baseline"], stream)
    return Spec("ds_bootstrap_counts_device", inputs, expect, call,
                outputs=dict(counts=(np.int64, c["n_boot"] * c["n_sets"] * 4), baseline=(np.int64, c["n_sets"] * 4)))


def _metric_rows(seed):
    """10,000 rows whose 8,400 negatives span more than one sort tile of 8,192 keys; ties and a few NaNs."""
    rng = np.random.RandomState(seed)
    labels = np.zeros(10000, np.float32)
    labels[rng.permutation(10000)[:1600]] = 1
    scores = (rng.randint(-4000, 4000, 10000) / 512.0).astype(np.float32)
    scores[::333] = np.nan
    return scores, labels


def case_auc(oracle):
    import metrics_oracle
    scores, labels = _metric_rows(31)
    n = scores.shape[0]
    inputs = dict(scores=_pair(scores), labels=_pair(labels))

    def expect(v):
        return dict(out=np.array(metrics_oracle.auc_counts(v["scores"], v["labels"]), dtype=np.int64))

    def call(lib, h, p, stream):
        return lib.ds_auc_device(p["scores"], p["labels"], n, p["out"], stream)
    return Spec("ds_auc_device", inputs, expect, call, host_outputs=dict(out=(np.int64, 5)))


def case_weighted_logloss(oracle):
    import metrics_oracle
    margins, labels = _metric_rows(32)
    n, beta = margins.shape[0], 5.0
    inputs = dict(margins=_pair(margins), labels=_pair(labels))

    def expect(v):
        return dict(out=np.array(metrics_oracle.logloss_counts(v["margins"], v["labels"], beta), dtype=np.int64))

    def call(lib, h, p, stream):
        return lib.ds_weighted_logloss_device(p["margins"], p["labels"], n, beta, p["out"], stream)
    # the tolerance of tests/test_gpu_metrics.py: the sum within one quantum per row, the rows equal
    return Spec("ds_weighted_logloss_device", inputs, expect, call, host_outputs=dict(out=(np.int64, 2)),
                compare=dict(out=lambda got, want: got[1] == want[1] and abs(int(got[0]) - int(want[0])) <= int(want[1]) and
                             (got[2:].view(np.uint8) == POISON).all()))


def case_training_pairs(oracle):
    import training_set_oracle as ts
    n, top_n, sample_n, seed = 300, 20, 5, 0x5eed0123456789ab
    rng = np.random.RandomState(40)
    rows = np.stack([rng.choice(100000, top_n, replace=False) for _ in range(n)]).astype(np.int32)
    index = rng.randint(-2 ** 62, 2 ** 62, n).astype(np.int64)
    own = np.where(rng.rand(n) < 0.5, rows[np.arange(n), rng.randint(0, top_n, n)], -1).astype(np.int32)
    own[::7] = 100001                                                     # a truth row that is no candidate
    inputs = dict(rows=_pair(rows), index=_pair(index), own=_pair(own))

    def expect(v):
        pair_t, target = [], []
        for q in range(n):
            sample, hit = ts.sample_candidates(v["rows"][q].tolist(), sample_n, int(v["own"][q]), seed, int(v["index"][q]))
            pair_t += sample
            target += hit
        return dict(pair_q=np.repeat(np.arange(n, dtype=np.int32), sample_n), pair_t=np.array(pair_t, dtype=np.int32),
                    target=np.array(target, dtype=np.float32))

    def call(lib, h, p, stream):
        return lib.ds_training_pairs_device(p["rows"], n, top_n, sample_n, p["index"], p["own"], ctypes.c_uint64(seed), 0,
                                            p["pair_q"], p["pair_t"], p["target"], stream)
    return Spec("ds_training_pairs_device", inputs, expect, call,
                outputs=dict(pair_q=(np.int32, n * sample_n), pair_t=(np.int32, n * sample_n),
                             target=(np.float32, n * sample_n)))


def case_hard_negatives(oracle):
    import hard_cases as hc
    case = hc.CASES["k100_exclude"]
    n, k = case["rows"].shape
    capacity = n * case["hard_n"]
    inputs = dict(rows=_pair(case["rows"]), margins=_pair(case["margins"]), own=_pair(case["own"]),
                  exclude=_pair(case["exclude"]), total=_pair(np.zeros(1, dtype=np.int64)))
    mined = ("pair_q", "pair_t", "position", "margin")

    def expect(v):
        got = hc.mine_keys(v["rows"], v["margins"], v["own"], v["exclude"], case["n_truth"], case["hard_n"],
                           case["min_margin"], case["q_first"])
        return dict(zip(mined, got[:4]), total=np.array([got[4]], dtype=np.int64))

    def call(lib, h, p, stream):
        return lib.ds_hard_negatives_device(p["rows"], p["margins"], n, k, case["n_truth"], p["own"], p["exclude"],
                                            case["exclude"].shape[1], case["hard_n"], ctypes.c_float(case["min_margin"]),
                                            case["q_first"], p["offsets"], p["total"], capacity,
                                            *(p[name] for name in mined), stream)
    outputs = dict(zip(mined, ((np.int32, capacity), (np.int32, capacity), (np.int32, capacity), (np.float32, capacity))))
    outputs["offsets"] = (np.int64, n)
    return Spec("ds_hard_negatives_device", inputs, expect, call, outputs=outputs, inout=("total",), scratch=("offsets",))


def case_hard_total(oracle):
    inputs = dict(total=_pair(np.array([4321], dtype=np.int64)))

    def call(lib, h, p, stream):
        return lib.ds_hard_total(p["total"], _out_pointer(p["out"], ctypes.c_int64), stream)
    return Spec("ds_hard_total", inputs, lambda v: dict(out=v["total"].copy()), call, host_outputs=dict(out=(np.int64, 1)))


def case_gather_rows(oracle):
    n_src, n_rows, width = 1800, 1029, 66
    rng = np.random.RandomState(50)
    source = rng.rand(n_src, width).astype(np.float32)
    rows = rng.randint(1, n_src, n_rows).astype(np.int64)
    inputs = dict(source=_pair(source), rows=_pair(rows))

    def call(lib, h, p, stream):
        return lib.ds_gather_rows_device(p["source"], width, p["rows"], n_rows, n_src, p["picked"], stream)
    return Spec("ds_gather_rows_device", inputs, lambda v: dict(picked=v["source"][v["rows"]]), call,
                outputs=dict(picked=(np.float32, n_rows * width)))


def case_threshold_sweep(oracle):
    import sweep_cases
    n_queries, k = 257, 5
    queries = sweep_cases.make_queries(n_queries, k, 1000, seed=503)
    lev, prob = sweep_cases.GRID_3X7
    names = ("rows", "d", "r", "s", "probabilities", "exact", "actual")
    inputs = {name: _pair(array) for name, array in zip(names, queries)}
    # thresholds must ascend strictly: the decoy grids are other grids of the same shape
    inputs.update(lev=_pair(lev, lev - 7), prob=_pair(prob, prob * np.float32(0.5)),
                  counts=_pair(np.zeros(lev.shape[0] * prob.shape[0] * 4, dtype=np.int64)))

    def expect(v):
        counts = sweep_cases.sweep_counts(oracle, tuple(v[name] for name in names), v["lev"], v["prob"])
        return dict(counts=np.asarray(counts, dtype=np.int64))

    def call(lib, h, p, stream):
        return lib.ds_threshold_sweep_device(*(p[name] for name in names), n_queries, k, p["lev"], lev.shape[0], p["prob"],
                                             prob.shape[0], p["counts"], stream)
    return Spec("ds_threshold_sweep_device", inputs, expect, call, inout=("counts",))


# ---- rows that read title tables ------------------------------------------------------------------------------------------------

_shared = {}


def _forms():
    """tests/title_cases.py's launch-form tables, the rows of a k = 17 launch (units straddle queries) and their pairs."""
    if "forms" not in _shared:
        import title_cases as tc
        case = tc.forms_case()
        _shared["forms"] = (case, tc.forms_rows(case, 17, 0).astype(np.int32))
    return _shared["forms"]


def _title_handles(with_sort_key=False):
    def make():
        from doppel_speller_amd import _lib
        from doppel_speller_amd.feature_engineering import SORT_KEY, TitleTable
        case, _ = _forms()
        handles = dict(queries=TitleTable(case.q_enc, case.q_len), truth=TitleTable(case.t_enc, case.t_len, case.t_counts))
        if with_sort_key:
            handles["sort_key"] = _lib.DeviceArray.from_host(np.ascontiguousarray(SORT_KEY, dtype=np.uint8))
        return handles
    return make


def _sort_key():
    from doppel_speller_amd.feature_engineering import SORT_KEY
    return np.ascontiguousarray(SORT_KEY, dtype=np.uint8)


def case_construct_features(oracle):
    import title_cases as tc
    case, rows = _forms()
    n_queries, k = rows.shape
    n = rows.size

    def expect(v):
        bits = tc.expected_features(oracle, case, *tc.pairs_of_rows(v["pair_t"], 0))
        return dict(out=np.ascontiguousarray(bits, dtype=np.uint32).view(np.float32))

    def call(lib, h, p, stream):
        return lib.ds_construct_features_indexed_device(h["queries"].handle, h["truth"].handle, None, p["pair_t"], 0, k,
                                                        tc.SPACE, tc.N_TRUTH, n, p["out"], stream)
    return Spec("ds_construct_features_indexed_device", dict(pair_t=_pair(rows)), expect, call, make=_title_handles(),
                outputs=dict(out=(np.float32, n * tc.FEATURES)))


def case_close_matches(oracle):
    import title_cases as tc
    case, rows = _forms()
    n_queries, k = rows.shape
    threshold = 94

    def expect(v):
        ratios = tc.expected_ratios(oracle, case, *tc.pairs_of_rows(v["rows"], 0), threshold, _sort_key())
        best = tc.best_from_ratios(ratios.reshape(n_queries, k), v["rows"], threshold)
        return dict(ratios=np.asarray(ratios, dtype=np.uint8), best=np.asarray(best, dtype=np.int32))

    def call(lib, h, p, stream):
        return lib.ds_close_matches_device(h["queries"].handle, h["truth"].handle, p["rows"], 0, k, n_queries, tc.SPACE,
                                           h["sort_key"].ptr, threshold, p["ratios"], p["best"], stream)
    return Spec("ds_close_matches_device", dict(rows=_pair(rows)), expect, call, make=_title_handles(True),
                outputs=dict(ratios=(np.uint8, n_queries * k), best=(np.int32, n_queries)))


def case_close_parts(oracle):
    import sweep_cases
    import title_cases as tc
    case, rows = _forms()
    n_queries, k = rows.shape
    t_min, t_max = 50, 94

    def expect(v):
        parts = sweep_cases.case_parts(oracle, case, *tc.pairs_of_rows(v["rows"], 0), _sort_key())
        return dict(zip("drs", sweep_cases.skipped_parts(*parts, t_min, t_max)))

    def call(lib, h, p, stream):
        return lib.ds_close_parts_device(h["queries"].handle, h["truth"].handle, p["rows"], 0, k, n_queries, tc.SPACE,
                                         h["sort_key"].ptr, t_min, t_max, p["d"], p["r"], p["s"], stream)
    return Spec("ds_close_parts_device", dict(rows=_pair(rows)), expect, call, make=_title_handles(True),
                outputs={name: (np.uint8, n_queries * k) for name in "drs"})


def case_exact_matches(oracle):
    """The exact-match table is built by the first call, on the call's stream, behind the gate."""
    import query_cases as qc
    _, truth, queries = next(table for table in qc.exact_tables() if table[0] == "1024")
    first, n = 123, len(queries) - 123 - 7
    exact = qc.exact_expected(truth, queries)[first:first + n]
    best = np.where(np.arange(n) % 3 == 0, -1, 5 + np.arange(n)).astype(np.int32)

    def make():
        import doppel_speller_amd as ds
        return dict(truth=ds.TitleTable(*qc.encode(truth)), queries=ds.TitleTable(*qc.encode(queries)))

    def expect(v):
        return dict(exact_row=exact, best=np.where(exact >= 0, exact, v["best"]).astype(np.int32))

    def call(lib, h, p, stream):
        return lib.ds_exact_matches_device(h["truth"].handle, h["queries"].handle, first, n, p["exact_row"], p["best"],
                                           stream)
    return Spec("ds_exact_matches_device", dict(best=_pair(best)), expect, call, make=make, inout=("best",),
                outputs=dict(exact_row=(np.int32, n)))


def case_query_rows(oracle):
    import query_cases as qc
    first, n = 5, 1029                        # past the scan's 1,024 titles
    if "query_rows" not in _shared:
        titles, _ = qc.rows_titles()
        keys, idf32, idf64 = qc.vocabulary(qc.truth_titles())
        enc, lengths = qc.encode(titles)
        _shared["query_rows"] = (titles, (keys, idf32, idf64),
                                 qc.rule_rows(enc[first:first + n], lengths[first:first + n], keys, idf32, idf64))
    titles, space_arrays, (rowptr, cols, maxint) = _shared["query_rows"]

    def make():
        import doppel_speller_amd as ds
        from doppel_speller_amd.prediction import QuerySpace
        return dict(space=QuerySpace(*space_arrays), titles=ds.TitleTable(*qc.encode(titles)))

    def expect(v):
        return dict(rowptr=np.asarray(rowptr, dtype=np.int64), cols=np.asarray(cols, dtype=np.int32),
                    maxint=np.asarray(maxint, dtype=np.float64))

    def call(lib, h, p, stream):
        return lib.ds_query_rows_device(h["space"].handle, h["titles"].handle, first, n, p["rowptr"], p["cols"],
                                        p["maxint"], 253 * n, stream)
    return Spec("ds_query_rows_device", {}, expect, call, make=make,
                outputs=dict(rowptr=(np.int64, n + 1), cols=(np.int32, 253 * n), maxint=(np.float64, n)))


# ---- rows that read a forest ------------------------------------------------------------------------------------------------------

def _forest_model(forest, n_features):
    def make():
        from doppel_speller_amd.forest import ForestModel
        return dict(model=ForestModel(forest["feature"], forest["threshold"], forest["yes"], forest["no"],
                                      forest["missing"], forest["tree_offsets"], n_features, forest["base_margin"]))
    return make


def _forest_and_rows(n=1000):
    if "forest" not in _shared:
        import contributions_cases as cc
        from doppel_speller_amd.forest import ForestModel
        forest = ForestModel.parse_xgboost_dump(cc.random_dump(31, n_trees=60, n_features=66, depth=6))
        rng = np.random.RandomState(33)
        rows = rng.uniform(0, 100, (n, 66)).astype(np.float32)
        rows[:, :6] = rng.randint(0, 100, (n, 6))
        rows[rng.rand(n, 66) < 0.1] = np.nan
        _shared["forest"] = (forest, rows)
    return _shared["forest"]


def case_forest_predict(oracle):
    forest, rows = _forest_and_rows()
    n = rows.shape[0]

    def expect(v):
        margins, probabilities = oracle.forest_predict(forest, v["rows"])
        return dict(margins=np.asarray(margins, dtype=np.float32), probabilities=np.asarray(probabilities, dtype=np.float32))

    def call(lib, h, p, stream):
        return lib.ds_forest_predict_device(h["model"].handle, p["rows"], n, p["margins"], p["probabilities"], stream)
    # the margins bit for bit; the probabilities as tests/test_gpu_forest.py holds them: float32 exp, device against libm
    return Spec("ds_forest_predict_device", dict(rows=_pair(rows)), expect, call, make=_forest_model(forest, 66),
                outputs=dict(margins=(np.float32, n), probabilities=(np.float32, n)),
                compare=dict(probabilities=lambda got, want: np.allclose(got[:n], want, rtol=3e-7, atol=0) and
                             (got[n:].view(np.uint8) == POISON).all()))


def case_forest_cover(oracle):
    """The counters are the forest's own: they are read back (ds_forest_cover_read) behind the call's completion.  Calls
    accumulate, so the second call on the same forest doubles them."""
    import contributions_cases as cc
    forest, rows = _forest_and_rows()
    n, n_nodes = rows.shape[0], forest["feature"].shape[0]

    def collect(lib, h, p):
        assert lib.ds_forest_cover_read(h["model"].handle, p["cover"]) == 0, lib.ds_last_error()

    def call(lib, h, p, stream):
        return lib.ds_forest_cover_device(h["model"].handle, p["rows"], n, stream)
    return Spec("ds_forest_cover_device", dict(rows=_pair(rows)),
                lambda v: dict(cover=cc.node_counts(forest, v["rows"]).astype(np.float64)), call,
                make=_forest_model(forest, 66), host_outputs=dict(cover=(np.float64, n_nodes)), collect=collect,
                expect_second=lambda v: dict(cover=2.0 * cc.node_counts(forest, v["rows"]).astype(np.float64)))


def case_forest_contributions(oracle):
    """The first call on a forest derives the TreeSHAP path tables from the cover (host work, uploads, one
    synchronisation); the second only enqueues."""
    import contributions_cases as cc
    forest, rows = _forest_and_rows()
    rows = rows[:200]
    n, width = rows.shape[0], 67
    if "cover" not in _shared:
        background = np.random.RandomState(32).uniform(0, 100, (5000, 66)).astype(np.float32)
        _shared["cover"] = cc.node_counts(forest, background).astype(np.float64) + 1.0 * _leaves_below(forest)
    cover = _shared["cover"]
    tolerance = cc.TOL_FACTOR * cc.forest_scale(forest)

    def make():
        handles = _forest_model(forest, 66)()
        handles["model"].set_cover(cover)
        return handles

    def call(lib, h, p, stream):
        return lib.ds_forest_contributions_device(h["model"].handle, p["rows"], n, p["out"], 0, stream)
    # the tolerance of tests/test_gpu_contributions.py: 1e-10 * (|base margin| + the sum over the trees of max |leaf|)
    return Spec("ds_forest_contributions_device", dict(rows=_pair(rows)),
                lambda v: dict(out=cc.tree_shap(forest, cover, v["rows"])), call, make=make,
                outputs=dict(out=(np.float64, n * width)),
                compare=dict(out=lambda got, want: bool(np.abs(got[:want.shape[0]] - want).max() <= tolerance) and
                             (got[want.shape[0]:].view(np.uint8) == POISON).all()))


def _leaves_below(forest):
    """The leaves below every node (forest.cover_from_counts' prior keeps a parent the sum of its children)."""
    feature, offsets = forest["feature"], forest["tree_offsets"]
    leaves = np.zeros(feature.shape[0], dtype=np.float64)
    for t in range(offsets.shape[0] - 1):
        begin, end = int(offsets[t]), int(offsets[t + 1])
        for i in range(end - 1, begin - 1, -1):
            leaves[i] = 1.0 if feature[i] < 0 else leaves[begin + forest["yes"][i]] + leaves[begin + forest["no"][i]]
    return leaves


def case_forest_inspect(oracle):
    import inspect_cases
    from doppel_speller_amd.forest import inspection_jobs
    c = inspect_cases.case("three_row_blocks")
    n, jobs = c["rows"].shape[0], inspection_jobs(c["jobs"])
    n_jobs = jobs.shape[0]
    import forest_inspect_oracle

    def expect(v):
        listed = [tuple(job) for job in v["jobs"].view(jobs.dtype).tolist()]
        counters, _ = forest_inspect_oracle.inspect(c["forest"], v["rows"], v["target"], listed, c["seed"],
                                                    inspect_cases.THRESHOLD)
        return dict(out=np.asarray(counters, dtype=np.uint64))

    def call(lib, h, p, stream):
        return lib.ds_forest_inspect_device(h["model"].handle, p["rows"], n, p["target"], p["jobs"], n_jobs, c["seed"],
                                            inspect_cases.THRESHOLD, p["out"], stream)
    # zero bytes are baseline jobs
    inputs = dict(rows=_pair(c["rows"]), target=_pair(c["target"]), jobs=_pair(jobs.view(np.uint8)))
    return Spec("ds_forest_inspect_device", inputs, expect, call, make=_forest_model(c["forest"], c["n_features"]),
                outputs=dict(out=(np.uint64, n_jobs * 5)))


def case_feature_cuts(oracle):
    import cuts_cases
    from doppel_speller_amd.train import compute_cuts
    features, _ = cuts_cases.crafted_matrix()
    features = np.ascontiguousarray(features, dtype=np.float32)
    n, n_features = features.shape
    max_bin = 256

    def expect(v):
        cuts, offsets = compute_cuts(v["features"], max_bin)
        return dict(cuts=np.asarray(cuts, dtype=np.float32), offsets=np.asarray(offsets, dtype=np.int32))

    def call(lib, h, p, stream):
        return lib.ds_feature_cuts_device(p["features"], n, n_features, max_bin, p["cuts"], p["offsets"], 0, stream)
    return Spec("ds_feature_cuts_device", dict(features=_pair(features)), expect, call,
                host_outputs=dict(cuts=(np.float32, n_features * 254), offsets=(np.int32, n_features + 1)))


# ---- Jaccard top-k and its two read-backs --------------------------------------------------------------------------------------

def _jaccard():
    """tests/test_gpu_jaccard.py's small-max-intersection problem: every second query has a q_maxint below its columns'
    idf total and is handed to the literal kernel (status 1), the others stay with the fast kernel (status 0).  The decoy
    is the same queries in reverse order: an accepted input of the same shape with another answer."""
    if "jaccard" not in _shared:
        import jaccard_cases as jc
        case = jc.random_problem(np.random.RandomState(79), 30000, 600, 32)
        case["q_maxint"] = case["q_maxint"].copy()
        case["q_maxint"][::2] *= 0.25
        lists = np.split(case["q_cols"], case["q_rowptr"][1:-1])[::-1]
        reverse = dict(q_rowptr=np.concatenate(([0], np.cumsum([len(c) for c in lists]))).astype(np.int64),
                       q_cols=np.concatenate(lists).astype(np.int32), q_maxint=case["q_maxint"][::-1].copy())
        _shared["jaccard"] = (case, reverse)
    return _shared["jaccard"]


def _jaccard_spec(oracle, entry):
    case, reverse = _jaccard()
    n_queries, k = case["q_maxint"].shape[0], case["k"]
    names = ("q_rowptr", "q_cols", "q_maxint")
    dtypes = (np.int64, np.int32, np.float64)
    inputs = {name: _pair(case[name], reverse[name], dtype=dtype) for name, dtype in zip(names, dtypes)}
    idf64 = case["idf32"].astype(np.float64)

    def make():
        from doppel_speller_amd.match_maker import TruthIndex
        return dict(index=TruthIndex(case["rowptr"], case["truth_idx"], case["idf32"], case["sums32"]))

    def expect(v):
        rows = oracle.jaccard_topk(case["rowptr"], case["truth_idx"], case["idf32"], case["sums32"], v["q_rowptr"],
                                   v["q_cols"], v["q_maxint"], k)
        want = dict(rows=np.asarray(rows, dtype=np.int32))
        if entry == "ds_jaccard_sync":
            want["stats"] = np.zeros(32, dtype=np.int64)
        if entry == "ds_jaccard_status":
            totals = np.array([idf64[c].sum() for c in np.split(v["q_cols"], v["q_rowptr"][1:-1])])
            want["status"] = (v["q_maxint"] < 0.5 * totals).astype(np.int32)        # these are handed over for certain
        return want

    def call(lib, h, p, stream):
        status = lib.ds_jaccard_topk_device(h["index"].handle, p["q_rowptr"], p["q_cols"], p["q_maxint"], n_queries, k,
                                            p["rows"], stream)
        if status == 0 and entry == "ds_jaccard_sync":
            status = lib.ds_jaccard_sync(h["index"].handle, stream, _out_pointer(p["stats"], ctypes.c_int64))
        if status == 0 and entry == "ds_jaccard_status":
            status = lib.ds_jaccard_status(h["index"].handle, stream, p["status"], n_queries)
        return status
    host, compare = {}, {}
    if entry == "ds_jaccard_sync":       # stats[0] the queries the literal kernel answered, [1] the queries in error
        host["stats"] = (np.int64, 32)
        compare["stats"] = lambda got, want: got[1] == 0 and n_queries // 2 <= got[0] < n_queries and \
            (got[32:].view(np.uint8) == POISON).all()
    if entry == "ds_jaccard_status":     # both kinds of query are there: 0 (fast kernel) and 1 (handed over)
        host["status"] = (np.int32, n_queries)
        compare["status"] = lambda got, want: set(got[:n_queries].tolist()) == {0, 1} and \
            (got[:n_queries] >= want).all() and (got[n_queries:].view(np.uint8) == POISON).all()
    return Spec(entry, inputs, expect, call, make=make, outputs=dict(rows=(np.int32, n_queries * k)), host_outputs=host,
                compare=compare)


def case_jaccard_topk(oracle):
    return _jaccard_spec(oracle, "ds_jaccard_topk_device")


def case_jaccard_sync(oracle):
    return _jaccard_spec(oracle, "ds_jaccard_sync")


def case_jaccard_status(oracle):
    return _jaccard_spec(oracle, "ds_jaccard_status")


# ---- rows that make or refill a handle -------------------------------------------------------------------------------------------

def _read_table(lib, handle, p):
    """ds_titles_read of a table the call made, into the host outputs `enc` and `len`; the table is destroyed."""
    try:
        assert lib.ds_titles_read(handle, p["enc"], p["len"]) == 0, lib.ds_last_error()
    finally:
        lib.ds_titles_destroy(handle)


def case_misspell_titles(oracle):
    import training_set_oracle as ts
    seed, n = 0x5eed0123456789ab, 200
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "misspell_matrix.npz")
    with np.load(golden, allow_pickle=False) as g:
        every = [bytes(x).decode("utf-8") for x in g["titles"]]
    titles = [every[i] for i in np.linspace(0, len(every) - 1, 300).astype(int)]
    rows = np.random.RandomState(5).permutation(300)[:n].astype(np.int32)

    def encode(strings):
        enc = np.zeros((len(strings), 255), dtype=np.uint8)
        for i, title in enumerate(strings):
            enc[i, :len(title)] = ts.to_codes(title)
        return enc, np.array([len(t) for t in strings], dtype=np.uint8)

    def make():
        import doppel_speller_amd as ds
        return dict(source=ds.TitleTable(*encode(titles)))

    def expect(v):
        enc, lengths = encode([ts.misspell(titles[r], seed, int(r)) for r in v["rows"]])
        return dict(enc=enc, len=lengths)

    def call(lib, h, p, stream):
        h["made"] = ctypes.c_void_p()
        return lib.ds_misspell_titles(h["source"].handle, p["rows"], n, ctypes.c_uint64(seed), stream,
                                      ctypes.byref(h["made"]))
    return Spec("ds_misspell_titles", dict(rows=_pair(rows)), expect, call, make=make,
                host_outputs=dict(enc=(np.uint8, n * 255), len=(np.uint8, n)),
                collect=lambda lib, h, p: _read_table(lib, h["made"], p))


def case_prepare_titles(oracle):
    """Host titles in, a table out: nothing to stage, the table must be complete when the call returns."""
    import query_cases as qc
    titles = [title for _, title in qc.fixed_titles()]
    raw = [t.encode("ascii") for t in titles]
    offsets = np.zeros(len(raw) + 1, dtype=np.int64)
    np.cumsum([len(t) for t in raw], out=offsets[1:])
    chars = np.frombuffer(b"".join(raw), dtype=np.uint8)
    n = len(raw)

    def expect(v):
        from doppel_speller_amd import prediction
        from doppel_speller_amd.feature_engineering import encode_collection
        enc, lengths = encode_collection(*prediction._pack([oracle.transform_title(t) for t in titles]),
                                         prediction._CODE_OF)
        return dict(enc=np.ascontiguousarray(enc, dtype=np.uint8), len=np.ascontiguousarray(lengths, dtype=np.uint8),
                    report=np.array([-1, -1], dtype=np.int64))

    def call(lib, h, p, stream):
        from doppel_speller_amd import _lib
        h["made"] = ctypes.c_void_p()
        return lib.ds_prepare_titles(_lib.pointer(chars), _lib.pointer(offsets), n, 1, 0, stream, ctypes.byref(h["made"]),
                                     p["report"])
    # report[0..1] is the mask of refused bytes (the catalogue's own test pins it), [2] and [3] the rows in error: none
    return Spec("ds_prepare_titles", {}, expect, call, host_outputs=dict(enc=(np.uint8, n * 255), len=(np.uint8, n),
                                                                         report=(np.int64, 4)),
                collect=lambda lib, h, p: _read_table(lib, h["made"], p),
                compare=dict(report=lambda got, want: got[2:4].tolist() == want.tolist() and
                             (got[4:].view(np.uint8) == POISON).all()))


def case_exhaustive_rank(oracle):
    import exhaustive_cases as ec
    import title_cases as tc
    case, _ = _forms()
    forest, _ = _forest_and_rows()
    q_first, n_queries, n = 3, 2, 5

    def make():
        handles = _title_handles()()
        handles.update(_forest_model(forest, 66)())
        return handles

    def expect(v):
        if "exhaustive" not in _shared:
            pair_q = np.repeat(np.arange(q_first, q_first + n_queries, dtype=np.int64), case.n_t)
            pair_t = np.tile(np.arange(case.n_t, dtype=np.int64), n_queries)
            features = tc.expected_features(oracle, case, pair_q, pair_t).view(np.float32)
            probabilities = oracle.forest_predict(forest, np.ascontiguousarray(features))[1]
            _shared["exhaustive"] = ec.best_rows(np.asarray(probabilities, np.float32).reshape(n_queries, case.n_t), n)
        rows, probabilities = _shared["exhaustive"]
        return dict(out_row=np.asarray(rows, dtype=np.int32), out_probability=np.asarray(probabilities, dtype=np.float32))

    def call(lib, h, p, stream):
        return lib.ds_exhaustive_rank_device(h["queries"].handle, h["truth"].handle, h["model"].handle, q_first, n_queries,
                                             n, tc.SPACE, tc.N_TRUTH, p["out_row"], p["out_probability"], stream)
    return Spec("ds_exhaustive_rank_device", {}, expect, call, make=make,
                outputs=dict(out_row=(np.int32, n_queries * n), out_probability=(np.float32, n_queries * n)))


def _training_data():
    if "training" not in _shared:
        import forest_continue_oracle as continued
        from forest_train_oracle import make_data
        from doppel_speller_amd.train import compute_cuts
        x, y = make_data(3000, 6, 11)
        x, y = np.ascontiguousarray(x, dtype=np.float32), np.ascontiguousarray(y, dtype=np.float32)
        forest = continued.flat_forest(continued.random_forest(5, 3, 6, seed=3))
        _shared["training"] = (x, y, forest, compute_cuts(x, 256))
    return _shared["training"]


def _seed_spec(entry):
    """A trainer binned from the real matrix; the seed call then walks the forest over the STAGED raw matrix.  Seeding is
    legal once per trainer, so the second call runs on a second fresh trainer."""
    import forest_continue_oracle as continued
    x, y, forest, (cuts, cut_offsets) = _training_data()
    n, n_features = x.shape
    batch = entry == "ds_trainer_batch_seed_device"
    fold = (np.arange(n) % 2).astype(np.uint8)
    params = np.array([3, 0.1, 1.0, 1.0, 5.0] * 2, dtype=np.float64)
    held_out = np.array([0, 1], dtype=np.int32)

    def make():
        from doppel_speller_amd import _lib
        lib, pointer = _lib.lib(), _lib.pointer
        handles = _forest_model(forest, n_features)()
        handles["trainer"] = ctypes.c_void_p()
        if batch:
            _lib.check(lib.ds_trainer_batch_create(pointer(x), n, n_features, pointer(cuts), pointer(cut_offsets), pointer(y),
                                                   pointer(fold), 2, 2, pointer(params), pointer(held_out), 0,
                                                   ctypes.byref(handles["trainer"])), "ds_trainer_batch_create")
        else:
            _lib.check(lib.ds_trainer_create(pointer(x), n, n_features, pointer(cuts), pointer(cut_offsets), 3, 0.1, 1.0, 1.0,
                                             5.0, 0, ctypes.byref(handles["trainer"])), "ds_trainer_create")
            _lib.check(lib.ds_trainer_set_labels(handles["trainer"], pointer(y)), "ds_trainer_set_labels")
        return handles

    def call(lib, h, p, stream):
        if batch:
            return lib.ds_trainer_batch_seed_device(h["trainer"], h["model"].handle, p["features"], None, stream)
        return lib.ds_trainer_seed_device(h["trainer"], h["model"].handle, p["features"], None, None, stream)

    def collect(lib, h, p):
        try:
            if batch:        # the margins of the second model: all rows, held-out ones included
                assert lib.ds_trainer_batch_read(h["trainer"], 1, p["margins"], None, None, None) == 0, lib.ds_last_error()
            else:
                assert lib.ds_trainer_read(h["trainer"], p["margins"], None, None, None, None) == 0, lib.ds_last_error()
        finally:
            (lib.ds_trainer_batch_destroy if batch else lib.ds_trainer_destroy)(h["trainer"])
            h["trainer"] = None
    return Spec(entry, dict(features=_pair(x)),
                lambda v: dict(margins=(np.float32(0.0) + continued.leaf_sums(forest, v["features"])).astype(np.float32)),
                call, make=make, host_outputs=dict(margins=(np.float32, n)), collect=collect, once=True)


def case_trainer_seed(oracle):
    return _seed_spec("ds_trainer_seed_device")


def case_trainer_batch_seed(oracle):
    return _seed_spec("ds_trainer_batch_seed_device")


def case_forest_refresh(oracle):
    """refresh_leaf = 0: every leaf keeps its value, so the leaves and the margins are the forest's own, bit for bit.  The
    gradient sums depend on p = 1.0f / (1.0f + expf(-m)), which the device and NumPy round differently: 2^-22 relative on
    the device (tests/test_gpu_refresh.py derives it), a few steps in NumPy's float32 exp; g and h are at most max(beta, 1)
    times p, in units of 2^-30: under 5 * 2^30 * 2^-21 < 4096 units a row, so a node's sums are held to 4096 units times
    the rows of the matrix."""
    import forest_refresh_oracle
    x, y, forest, _ = _training_data()
    n, n_features = x.shape
    n_nodes, n_trees = forest["feature"].shape[0], forest["tree_offsets"].shape[0] - 1
    slack = 4096 * n

    def expect(v):
        want = forest_refresh_oracle.refresh(forest, v["features"], y, eta=0.1, reg_lambda=1.0, beta=5.0,
                                             refresh_leaf=False)
        return dict(leaf_out=np.asarray(want["leaves"], dtype=np.float32),
                    node_sums=np.asarray(want["node_sums"], dtype=np.int64),
                    margins=np.asarray(want["margins"], dtype=np.float32),
                    empty=np.array([want["empty_leaves"]], dtype=np.int64))

    def call(lib, h, p, stream):
        from doppel_speller_amd import _lib
        return lib.ds_forest_refresh_device(h["model"].handle, p["features"], n, _lib.pointer(y), None, None, None, 0, 0.1,
                                            1.0, 5.0, 0, p["leaf_out"], p["node_sums"], p["margins"], p["errors"],
                                            _out_pointer(p["empty"], ctypes.c_int64), None, stream)
    return Spec("ds_forest_refresh_device", dict(features=_pair(x)), expect, call, make=_forest_model(forest, n_features),
                host_outputs=dict(leaf_out=(np.float32, n_nodes), node_sums=(np.int64, 2 * n_nodes), margins=(np.float32, n),
                                  errors=(np.int64, n_trees + 1), empty=(np.int64, 1)),
                scratch=("errors",),
                compare=dict(node_sums=lambda got, want: bool(np.abs(got[:want.shape[0]] - want).max() <= slack) and
                             (got[want.shape[0]:].view(np.uint8) == POISON).all()))


CASES = {
    "ds_jaccard_topk_device": case_jaccard_topk,
    "ds_jaccard_sync": case_jaccard_sync,
    "ds_jaccard_status": case_jaccard_status,
    "ds_misspell_titles": case_misspell_titles,
    "ds_prepare_titles": case_prepare_titles,
    "ds_exhaustive_rank_device": case_exhaustive_rank,
    "ds_trainer_seed_device": case_trainer_seed,
    "ds_trainer_batch_seed_device": case_trainer_batch_seed,
    "ds_forest_refresh_device": case_forest_refresh,
    "ds_construct_features_indexed_device": case_construct_features,
    "ds_close_matches_device": case_close_matches,
    "ds_close_parts_device": case_close_parts,
    "ds_exact_matches_device": case_exact_matches,
    "ds_query_rows_device": case_query_rows,
    "ds_forest_predict_device": case_forest_predict,
    "ds_forest_cover_device": case_forest_cover,
    "ds_forest_contributions_device": case_forest_contributions,
    "ds_forest_inspect_device": case_forest_inspect,
    "ds_feature_cuts_device": case_feature_cuts,
    "ds_rank_matches_device": case_rank_matches,
    "ds_assign_edges_device": case_assign_edges,
    "ds_assign_solve_device": case_assign_solve,
    "ds_remaining_pairs_device": case_remaining_pairs,
    "ds_select_matches_device": case_select_matches,
    "ds_exhaustive_fold_device": case_exhaustive_fold,
    "ds_exhaustive_finish_device": case_exhaustive_finish,
    "ds_duplicate_begin_device": case_duplicate_begin,
    "ds_duplicate_links_device": case_duplicate_links,
    "ds_duplicate_finish_device": case_duplicate_finish,
    "ds_best_pairs_device": case_best_pairs,
    "ds_outcome_codes_device": case_outcome_codes,
    "ds_calibration_apply_device": case_calibration_apply,
    "ds_reliability_device": case_reliability,
    "ds_isotonic_fit_device": case_isotonic_fit,
    "ds_bootstrap_counts_device": case_bootstrap_counts,
    "ds_auc_device": case_auc,
    "ds_weighted_logloss_device": case_weighted_logloss,
    "ds_training_pairs_device": case_training_pairs,
    "ds_hard_negatives_device": case_hard_negatives,
    "ds_hard_total": case_hard_total,
    "ds_gather_rows_device": case_gather_rows,
    "ds_threshold_sweep_device": case_threshold_sweep,
}
NOT_COVERED = {}
