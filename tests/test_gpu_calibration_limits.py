"""The launch paths of csrc/ds_calibrate.hip that tests/test_gpu_calibration.py does not take, bit for bit against
tests/calibration_oracle.py: the pool kernel with more dynamic LDS than the 48 KiB a kernel gets unasked
(segment_points = 2048: 52,224 B), the map with its edges staged in LDS beyond 48 KiB (12,288 < K <= 16,384) on both
sides of both limits, and a fit of more than 2048 * 1024 rows, where the scan of the head tiles' totals takes a second
trip through its loop."""
import numpy as np
import pytest

import calibration_cases as cases
import calibration_oracle as oracle
from test_gpu_calibration import device_apply, device_fit, host_fit, options, same

pytestmark = pytest.mark.gpu

FIT_CASES = cases.fit_cases()
HEAD_TILE, SCAN_THREADS = 2048, 1024           # kCalibrateHeadTile, kScanThreads
BIG_ROWS = HEAD_TILE * SCAN_THREADS + HEAD_TILE + 3


@pytest.mark.parametrize("name", ["staircase", "staircase_then_negatives", "random_20000"])
def test_the_widest_segment_needs_the_lds_opt_in(name):
    """W = 2048: six arrays of W + 128 words.  `staircase` is 3043 points that pool nothing: two segments, and a stack
    of the last level deeper than its part in LDS."""
    scores, target = FIT_CASES[name]
    want = oracle.fit(scores, target)
    if name == "staircase":
        assert want["n_points"] == want["lo"].shape[0] == 3043
    default = device_fit(scores, target)
    same(default, want, "default")
    with options(segment_points=2048):
        wide = device_fit(scores, target)
        same(wide, want, "segment_points=2048")
        same(host_fit(scores, target), want, "segment_points=2048, host")
    with options(segment_points=2048, max_blocks=1):
        same(device_fit(scores, target), want, "segment_points=2048, max_blocks=1")
    assert all(a.tobytes() == b.tobytes() for a, b in zip(default[1:5], wide[1:5]))
    assert int(wide[5][3]) <= int(default[5][3])       # wider segments leave no more blocks to the last level
    same(device_fit(scores, target), want, "default again")


@pytest.mark.parametrize("K", [12288, 12289, 16384, 16385])
def test_the_map_on_both_sides_of_its_two_lds_limits(K):
    """K edges of both signs, 4 K bytes of LDS: 48 KiB exactly, the first size that needs the opt-in, the last staged
    size, and the first that stays in HBM.  Every edge with its two float32 neighbours, and the ends."""
    lo = ((np.arange(K, dtype=np.float64) - K // 2) * 0.25).astype(np.float32)
    assert (np.diff(oracle.cut_key(lo).astype(np.int64)) > 0).all()
    value = (np.arange(1, K + 1, dtype=np.float64) / K).astype(np.float32)
    probes = np.concatenate([oracle.neighbours(lo), np.array([-np.inf, np.inf, -1e9, 1e9, 0.0, -0.0], np.float32)])
    mapped = oracle.transform(lo, value, probes)
    assert np.unique(mapped[~np.isnan(mapped)]).shape[0] == K + 1            # every block and the 0 below the first
    assert device_apply(lo, value, probes).tobytes() == mapped.tobytes()
    with options(max_blocks=1):
        assert device_apply(lo, value, probes).tobytes() == mapped.tobytes()
    assert device_apply(lo[:7], value[:7], probes).tobytes() == oracle.transform(lo[:7], value[:7], probes).tobytes()


def test_a_fit_of_more_head_tiles_than_the_tile_scan_has_threads():
    """2048 * 1024 + 2048 + 3 rows of 5000 distinct scores: 1026 head tiles, so the one workgroup that scans their totals
    carries its running sum into a second trip.  Once with the default grids and once with three workgroups striding
    over everything."""
    scores, target = cases._random(5, BIG_ROWS, 5000)
    assert (BIG_ROWS + 1 + HEAD_TILE - 1) // HEAD_TILE > SCAN_THREADS
    want = oracle.fit(scores, target)
    assert want["n_points"] == 5000 and want["n_nan"] == 0
    same(device_fit(scores, target), want, "default")
    with options(max_blocks=3):
        same(device_fit(scores, target), want, "max_blocks=3")
