"""Crafted float32 columns for the cut rule (DESIGN.md section 9 "Cuts"), shared by the CPU and GPU tests of
compute_cuts_device.  Every column is generated from a seed; nothing here calls the code under test."""
import numpy as np

ROWS = 6000


def _spread(values, rng):
    """ROWS entries that hold every one of `values` at least once, shuffled."""
    values = np.asarray(values, dtype=np.float32)
    column = values[np.arange(ROWS) % values.shape[0]]
    rng.shuffle(column)
    return column


def _from_bits(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def crafted_columns(seed=0):
    """name -> float32[ROWS], insertion-ordered."""
    rng = np.random.RandomState(seed)
    columns = {}
    for count in (1, 2, 14, 15, 16, 254, 255, 256):        # the distinct / quantile boundary of max_bin 2, 16, 256
        columns[f"distinct_{count}"] = _spread(rng.randn(count * 4).astype(np.float32)[:count] + np.arange(count), rng)
    columns["all_nan"] = np.full(ROWS, np.nan, np.float32)
    one = np.full(ROWS, np.nan, np.float32)
    one[ROWS // 3] = -2.5
    columns["one_value"] = one
    columns["all_equal"] = np.full(ROWS, 7.0, np.float32)
    columns["signed_zeros"] = _spread([-0.0, 0.0, -0.0, 0.0, -1.0, 1.0], rng)
    infinities = rng.randn(ROWS).astype(np.float32)
    infinities[rng.rand(ROWS) < 0.1] = np.inf
    infinities[rng.rand(ROWS) < 0.1] = -np.inf
    columns["infinities"] = infinities
    denormal = rng.randint(1, 1 << 23, ROWS).astype(np.uint32)           # exponent 0: denormals
    denormal[rng.rand(ROWS) < 0.5] |= np.uint32(0x80000000)
    denormal[::7] = (denormal[::7] & np.uint32(0x80000000)) | np.uint32(1 + (np.arange(denormal[::7].shape[0]) % 5))
    columns["denormals"] = _from_bits(denormal)
    columns["denormals_few"] = _spread(_from_bits([1, 2, 0x80000001, 0x80000002, 0, 0x80000000, 0x007fffff]), rng)
    # bits that share their two low bytes: all positive -> the two low digits are the same in every key and their
    # passes are skipped; with both signs the keys of the negative values carry the flipped bytes -> no pass is skipped
    high = rng.randint(0x3000, 0x5000, ROWS).astype(np.uint32) << np.uint32(16)
    columns["shared_low_positive"] = _from_bits(high | np.uint32(0x1234))
    sign = np.where(rng.rand(ROWS) < 0.5, np.uint32(0x80000000), np.uint32(0))
    columns["shared_low_mixed"] = _from_bits(high | np.uint32(0x1234) | sign)
    columns["shared_high"] = _from_bits(np.uint32(0x40490000) | rng.randint(0, 1 << 16, ROWS).astype(np.uint32))
    columns["small_integers"] = rng.randint(0, 21, ROWS).astype(np.float32)
    nan_30 = rng.randn(ROWS).astype(np.float32)
    nan_30[rng.rand(ROWS) < 0.3] = np.nan
    columns["nan_30"] = nan_30
    few_with_nan = _spread(np.arange(255, dtype=np.float32) - 100, rng)
    few_with_nan[rng.rand(ROWS) < 0.3] = np.nan
    few_with_nan[:255] = np.arange(255, dtype=np.float32) - 100
    columns["distinct_255_nan_30"] = few_with_nan
    columns["normal"] = rng.randn(ROWS).astype(np.float32)
    return columns


def crafted_matrix(seed=0):
    columns = crafted_columns(seed)
    return np.ascontiguousarray(np.column_stack(list(columns.values())), dtype=np.float32), list(columns)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
