"""ds_hard_negatives_device through the C ABI against the NumPy restatement of the rule (tests/hard_cases.py), bit for bit:
every named case as one call, with a grid of one workgroup that strides, cut into chunks that hand the running total on,
and with a capacity one short of the need."""
import ctypes

import numpy as np
import pytest

import hard_cases as hc
from doppel_speller_amd import _lib

pytestmark = pytest.mark.gpu

GUARD = 8                       # elements behind every output array that no call may touch
GUARD_BYTE = 0x55
DTYPES = (np.int32, np.int32, np.int32, np.float32)


@pytest.fixture
def max_blocks():
    """Sets the "max_blocks" cap for a test and puts the default back."""
    def choose(value):
        _lib.check(_lib.lib().ds_hard_option(b"max_blocks", value), "ds_hard_option")
    yield choose
    choose(0)


class Outputs:
    """The four mined arrays of `capacity` slots with a guard region behind each, and the running total."""

    def __init__(self, capacity):
        self.capacity = capacity
        self.arrays = [_lib.DeviceArray((capacity + GUARD,), dtype) for dtype in DTYPES]
        for array in self.arrays:
            _lib.check(_lib.lib().ds_memset(array.ptr, GUARD_BYTE, array.nbytes, 0), "ds_memset")
        self.total = _lib.DeviceArray.from_host(np.zeros(1, np.int64))

    def mine(self, case):
        """One call for the titles of `case`, appended behind the running total; no synchronisation."""
        n, k = case["rows"].shape
        # an empty chunk reads nothing: any non-null address will do
        inputs = [_lib.DeviceArray.from_host(case[name] if n else np.zeros(1, case[name].dtype))
                  for name in ("rows", "margins", "own")]
        exclude, n_exclude = case["exclude"], 0 if case["exclude"] is None else case["exclude"].shape[1]
        d_exclude = _lib.DeviceArray.from_host(exclude if n else np.zeros(1, np.int32)) if n_exclude else None
        offsets = _lib.DeviceArray((max(n, 1),), np.int64)
        _lib.check(_lib.lib().ds_hard_negatives_device(
            inputs[0].ptr, inputs[1].ptr, n, k, case["n_truth"], inputs[2].ptr, _lib.pointer(d_exclude), n_exclude,
            case["hard_n"], ctypes.c_float(case["min_margin"]), case["q_first"], offsets.ptr, self.total.ptr,
            self.capacity, *(a.ptr for a in self.arrays), None), "ds_hard_negatives_device")
        return inputs, d_exclude, offsets          # alive until the caller has synchronised

    def status(self):
        total = ctypes.c_int64(-1)
        return _lib.lib().ds_hard_total(self.total.ptr, ctypes.byref(total), None), int(total.value)

    def read(self):
        """(pair_q, pair_t, position, margin, total) and the bytes of the guard regions."""
        status, total = self.status()
        assert status == 0, _lib.lib().ds_last_error()
        whole = [a.to_host() for a in self.arrays]
        guards = [a[total:].view(np.uint8) for a in whole]      # the slots no pair took, and the region behind the array
        return tuple(a[:total] for a in whole) + (total,), guards


def _run(case, sizes=None):
    """The case in one call, or cut into chunks of the given sizes in turn."""
    n, expected = case["rows"].shape[0], hc.mine_keys(*hc.arguments(case))
    out, keep, first, turn = Outputs(n * case["hard_n"]), [], 0, 0
    while first < n or not keep:
        last = n if sizes is None else min(n, first + sizes[turn % len(sizes)])
        keep.append(out.mine(hc.chunk_of(case, first, last)))
        first, turn = last, turn + 1
    got, guards = out.read()
    assert all((g == GUARD_BYTE).all() for g in guards)
    return got, expected


@pytest.mark.parametrize("name", sorted(hc.CASES))
def test_every_case_in_one_call(name):
    got, expected = _run(hc.CASES[name])
    assert hc.same_mined(got, expected), name


@pytest.mark.parametrize("name", sorted(hc.CASES))
def test_every_case_with_a_grid_of_one_workgroup(name, max_blocks):
    max_blocks(1)
    got, expected = _run(hc.CASES[name])
    assert hc.same_mined(got, expected), name


@pytest.mark.parametrize("name", sorted(hc.CASES))
def test_every_case_cut_into_chunks(name):
    case = hc.CASES[name]
    for sizes in ((1,), (2,), (3,), (3, 1, 2)):
        got, expected = _run(case, sizes)
        assert hc.same_mined(got, expected), (name, sizes)


@pytest.mark.parametrize("name", ["k64_full", "k100_exclude", "k600_threshold", "nine_titles"])
def test_a_capacity_one_short_is_reported_and_nothing_is_written_past_it(name):
    case = hc.CASES[name]
    expected = hc.mine_keys(*hc.arguments(case))
    need, n = expected[4], case["rows"].shape[0]
    assert need >= 2
    for sizes in (None, (2,)):
        out, keep = Outputs(need - 1), []
        for first in range(0, n, n if sizes is None else sizes[0]):
            keep.append(out.mine(hc.chunk_of(case, first, n if sizes is None else min(n, first + sizes[0]))))
        status, total = out.status()
        assert status == -1 and total == need and b"more than the capacity" in _lib.lib().ds_last_error()
        whole = [a.to_host() for a in out.arrays]
        assert all((a[need - 1:].view(np.uint8) == GUARD_BYTE).all() for a in whole)
        # a later chunk does not bring the total back under the capacity
        keep.append(out.mine(hc.chunk_of(case, 0, 1)))
        status, total = out.status()
        assert status == -1 and total >= need
        assert all((a.to_host()[need - 1:].view(np.uint8) == GUARD_BYTE).all() for a in out.arrays)
    exact = Outputs(need)                                 # the exact capacity is enough
    keep.append(exact.mine(case))
    got, guards = exact.read()
    assert hc.same_mined(got, expected) and all((g == GUARD_BYTE).all() for g in guards)


def test_title_counts_past_the_grid(max_blocks):
    """One wave per title, four per workgroup, and a scan that takes 1024 titles a step: 4,099 titles on the default grid,
    on 3 workgroups that stride, and cut at 1,025."""
    base = hc.CASES["k100_exclude"]
    repeat = 456
    case = dict(base, rows=np.tile(base["rows"], (repeat, 1))[:4099], margins=np.tile(base["margins"], (repeat, 1))[:4099],
                own=np.tile(base["own"], repeat)[:4099], exclude=np.tile(base["exclude"], (repeat, 1))[:4099])
    for blocks, sizes in ((0, None), (3, None), (0, (1025,))):
        max_blocks(blocks)
        got, expected = _run(case, sizes)
        assert hc.same_mined(got, expected) and got[4] > 4099, (blocks, sizes)


def test_an_empty_chunk_keeps_the_total():
    case = hc.CASES["k5_own_first"]
    out = Outputs(12)
    keep = [out.mine(hc.chunk_of(case, 0, 2)), out.mine(hc.chunk_of(case, 2, 2)), out.mine(hc.chunk_of(case, 2, 4))]
    got, _ = out.read()
    assert hc.same_mined(got, hc.mine_keys(*hc.arguments(case))) and keep
