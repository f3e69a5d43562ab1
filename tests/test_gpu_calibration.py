"""The calibration kernels on the GPU ("Calibration"; csrc/ds_calibrate.hip) against the NumPy
restatement of the rule (tests/calibration_oracle.py).  Everything is integers or a look-up, so everything is compared
bit for bit: the level sets of every case through the C ABI in its device and host forms, under every segment width,
the map on every case's own scores and on every float32 neighbour of every edge, the reliability counters, two runs."""
import contextlib

import numpy as np
import pytest

import calibration_cases as cases
import calibration_oracle as oracle

pytestmark = pytest.mark.gpu

FIT_CASES = cases.fit_cases()
RELIABILITY_CASES = cases.reliability_cases()


@pytest.fixture(scope="module")
def expected():
    """The oracle's fit of every case, computed once."""
    return {name: oracle.fit(*FIT_CASES[name]) for name in FIT_CASES}


@contextlib.contextmanager
def options(**values):
    """ds_calibrate_option for the duration of a block; every option is back at its default afterwards."""
    from doppel_speller_amd import _lib
    try:
        for name, value in values.items():
            _lib.check(_lib.lib().ds_calibrate_option(name.encode(), value), "ds_calibrate_option")
        yield
    finally:
        for name in values:
            _lib.lib().ds_calibrate_option(name.encode(), 0)


def device_fit(scores, target):
    """ds_isotonic_fit_device -> (status, lo, hi, pos, neg, out[4]); the block arrays cut to K."""
    from doppel_speller_amd import _lib
    n = scores.shape[0]
    held = [_lib.DeviceArray.from_host(scores), _lib.DeviceArray.from_host(target)] if n else [None, None]
    held += [_lib.DeviceArray((max(n, 1),), dtype) for dtype in (np.float32, np.float32, np.int64, np.int64)]
    out = np.full(4, -1, np.int64)
    try:
        status = _lib.lib().ds_isotonic_fit_device(_lib.pointer(held[0]), _lib.pointer(held[1]), n, held[2].ptr,
                                                   held[3].ptr, held[4].ptr, held[5].ptr, _lib.pointer(out), None)
        blocks = int(out[0]) if status == 0 else 0
        return (status,) + tuple(array.to_host(blocks) for array in held[2:]) + (out,)
    finally:
        for array in held:
            if array is not None:
                array.free()


def host_fit(scores, target):
    from doppel_speller_amd import _lib
    n = scores.shape[0]
    room = max(n, 1)
    lo, hi = np.zeros(room, np.float32), np.zeros(room, np.float32)
    pos, neg, out = np.zeros(room, np.int64), np.zeros(room, np.int64), np.full(4, -1, np.int64)
    status = _lib.lib().ds_isotonic_fit(_lib.pointer(scores if n else None), _lib.pointer(target if n else None), n,
                                        _lib.pointer(lo), _lib.pointer(hi), _lib.pointer(pos), _lib.pointer(neg),
                                        _lib.pointer(out), 0)
    blocks = int(out[0]) if status == 0 else 0
    return status, lo[:blocks], hi[:blocks], pos[:blocks], neg[:blocks], out


def same(got, want, form):
    status, lo, hi, pos, neg, out = got
    assert status == 0, form
    assert int(out[0]) == want["lo"].shape[0], form
    assert int(out[1]) == want["n_nan"] and int(out[2]) == want["n_points"], form
    assert int(out[0]) <= int(out[3]) <= int(out[2]), form
    assert lo.dtype == np.float32 and lo.tobytes() == want["lo"].tobytes(), form
    assert hi.tobytes() == want["hi"].tobytes(), form
    assert pos.dtype == np.int64 and pos.tobytes() == want["pos"].tobytes(), form
    assert neg.tobytes() == want["neg"].tobytes(), form


@pytest.mark.parametrize("name", sorted(FIT_CASES))
def test_the_level_sets_equal_the_oracle_in_every_form(name, expected):
    """Segment widths 2 and 3 put a boundary between all neighbours, 64 gives every lane one point, and one workgroup
    strides over every grid; the default runs whole segments of 1024 points."""
    scores, target = FIT_CASES[name]
    want = expected[name]
    same(device_fit(scores, target), want, "device")
    same(host_fit(scores, target), want, "host")
    results = []
    for width in (2, 3, 64):
        with options(segment_points=width, max_blocks=1):
            results.append(device_fit(scores, target))
            same(results[-1], want, f"segment_points={width}")
    for other in results[1:]:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(results[0][1:5], other[1:5]))
    if name == "staircase_then_negatives":
        assert int(results[0][5][3]) > int(results[0][5][0])   # the last level had pooling left to do


def test_two_runs_give_the_same_bytes():
    scores, target = FIT_CASES["random_20000"]
    first, second = device_fit(scores, target), device_fit(scores, target)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first[1:], second[1:]))


def test_the_python_fit_returns_the_oracles_calibrator(expected):
    import doppel_speller_amd as ds
    for name in ("random_5000_nan", "empty", "nan_only", "extremes"):
        scores, target = FIT_CASES[name]
        want = expected[name]
        fitted = ds.fit_isotonic(scores, target)
        assert fitted == ds.Calibrator(want["lo"], want["hi"], want["pos"], want["neg"], want["n_nan"]), name
        assert fitted.values.tobytes() == oracle.values(want["pos"], want["neg"]).tobytes()
        assert fitted.n_rows == scores.shape[0] - want["n_nan"]


def device_apply(lo, value, scores):
    from doppel_speller_amd import _lib
    held = [_lib.DeviceArray.from_host(array) if array.shape[0] else None for array in (lo, value, scores)]
    d_out = _lib.DeviceArray((max(scores.shape[0], 1),), np.float32)
    try:
        _lib.check(_lib.lib().ds_calibration_apply_device(_lib.pointer(held[0]), _lib.pointer(held[1]), lo.shape[0],
                                                          _lib.pointer(held[2]), scores.shape[0], d_out.ptr, None),
                   "ds_calibration_apply_device")
        _lib.check(_lib.lib().ds_stream_sync(None, 0), "ds_stream_sync")
        return d_out.to_host(scores.shape[0])
    finally:
        for array in held + [d_out]:
            if array is not None:
                array.free()


@pytest.mark.parametrize("name", sorted(FIT_CASES))
def test_the_map_on_the_scores_and_on_every_neighbour_of_every_edge(name, expected):
    scores, _ = FIT_CASES[name]
    want = expected[name]
    value = oracle.values(want["pos"], want["neg"]).astype(np.float32)
    probes = np.concatenate([scores, oracle.neighbours(want["lo"]), oracle.neighbours(want["hi"]),
                             np.array([0.0, -0.0, np.inf, -np.inf], np.float32)])
    mapped = oracle.transform(want["lo"], value, probes)
    assert device_apply(want["lo"], value, probes).tobytes() == mapped.tobytes()
    with options(max_blocks=1):
        assert device_apply(want["lo"], value, probes).tobytes() == mapped.tobytes()


def test_the_map_reads_its_edges_from_hbm_beyond_the_staged_size():
    """More than 16384 blocks: the edges stay in HBM."""
    lo = np.arange(20001, dtype=np.float32)
    value = (np.arange(20001, dtype=np.float64) / 20001).astype(np.float32)
    probes = np.concatenate([oracle.neighbours(lo), np.array([-1.0, 1e9], np.float32)])
    assert device_apply(lo, value, probes).tobytes() == oracle.transform(lo, value, probes).tobytes()


def test_transform_device_equals_transform(expected):
    import doppel_speller_amd as ds
    from doppel_speller_amd import _lib
    scores, _ = FIT_CASES["random_5000_nan"]
    want = expected["random_5000_nan"]
    fitted = ds.Calibrator(want["lo"], want["hi"], want["pos"], want["neg"], want["n_nan"])
    d_scores, d_out = _lib.DeviceArray.from_host(scores), _lib.DeviceArray(scores.shape, np.float32)
    try:
        fitted.transform_device(d_scores, scores.shape[0], d_out)
        _lib.check(_lib.lib().ds_stream_sync(None, 0), "ds_stream_sync")
        got = d_out.to_host()
    finally:
        d_scores.free()
        d_out.free()
        fitted.free()
    assert got.tobytes() == fitted.transform(scores).tobytes()
    assert got.tobytes() == oracle.transform(want["lo"], fitted.values, scores).tobytes()


@pytest.mark.parametrize("name", sorted(RELIABILITY_CASES))
def test_the_reliability_counters_equal_the_oracle(name):
    import doppel_speller_amd as ds
    probabilities, target, n_bins = RELIABILITY_CASES[name]
    want = oracle.reliability(probabilities, target, n_bins)
    report = ds.reliability(probabilities, target, n_bins)
    assert report.counts.dtype == np.int64 and report.counts.tobytes() == want.tobytes()
    with options(max_blocks=1):
        assert ds.reliability(probabilities, target, n_bins).counts.tobytes() == want.tobytes()
    assert report.n_outside == int(want[n_bins, 0]) and report.n == int(want[:n_bins, 0].sum())
    if report.n:
        inside = (probabilities >= 0) & (probabilities <= 1)
        p, y = probabilities[inside].astype(np.float64), (target[inside] != 0).astype(np.float64)
        # the sums are quantised to 2^-30 per row: the mean is off by 2^-31 at the most
        assert abs(report.brier - float(((p - y) ** 2).mean())) <= 2.0 ** -31 + 1e-15
        assert 0.0 <= report.ece <= report.mce <= 1.0


def test_the_library_refuses_before_any_device_work():
    from doppel_speller_amd import _lib
    library, out = _lib.lib(), np.zeros(4, np.int64)
    assert library.ds_isotonic_fit_device(None, None, 5, None, None, None, None, _lib.pointer(out), None) == -1
    assert library.ds_isotonic_fit_device(None, None, 1 << 31, None, None, None, None, _lib.pointer(out), None) == -1
    assert library.ds_isotonic_fit_device(None, None, 0, None, None, None, None, _lib.pointer(out), None) == 0
    assert out.tolist() == [0, 0, 0, 0]
    assert library.ds_reliability_device(None, None, 0, 257, None, None) == -1
    assert library.ds_calibration_apply_device(None, None, 0, None, 3, None, None) == -1
    assert library.ds_calibrate_option(b"segment_points", 1) == -1
    assert library.ds_calibrate_option(b"no_such_option", 1) == -1
