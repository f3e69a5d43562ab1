"""NumPy restatement of the paired-bootstrap rule ("Is a difference real: the paired bootstrap"),
written from the rule's text, and the cases that test_bootstrap_cpu.py and test_gpu_bootstrap.py share.

    codes[m][i] in {0, 1, 2, 3}        the outcome class of row i under prediction set m
    unit[i] in [0, U), or none         the resampling unit of row i; none: U = n, every row its own unit
    T[u][m][c]                         the rows i with unit[i] == u and codes[m][i] == c
    baseline[m][c]                     the sum over u of T[u][m][c]
    x(b, k)                            the first kept output of the splitmix64 stream of (seed, purpose 7, (b << 32) | k)
    j(b, k) = (x * U) >> 64            the high 64 bits of the 128-bit product
    counts[b][m][c]                    the sum over k < U of T[j(b, k)][m][c], int64

Statistics on top, float64: error = class-2 count + weight * class-1 count; the interval at `level` is
np.quantile(errors[:, m], [(1 - level) / 2, (1 + level) / 2]); standard_error = errors.std(ddof=1), 0.0 for B = 1; the
difference of sets a and b is errors[:, a] - errors[:, b] replicate by replicate, with its mean, its interval and
share_better = (#{d < 0} + 0.5 * #{d == 0}) / B.
"""
import functools

import numpy as np

MASK = (1 << 64) - 1
PURPOSE_DRAW = 7
SETS_MAX, BOOT_MAX, ROWS_MAX = 64, 1 << 16, 1 << 31
LDS_TABLE_BYTES = 128 * 1024           # the largest table the kernel stages; a larger one is read from HBM
REPLICATES_PER_BLOCK = 4               # the launcher's default for up to 4096 replicates


# ---- the draws -----------------------------------------------------------------------------------------------------------
def stream_first(seed, purpose, index):
    """The first kept (third) output of the splitmix64 stream of (seed, purpose, index), in Python integers."""
    state = (seed * 0x9e3779b97f4a7c15 + index * 0xd1342543de82ef95 + purpose * 0xaf251af3b0f025b5) & MASK
    for _ in range(3):
        state = (state + 0x9e3779b97f4a7c15) & MASK
        z = state
        z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & MASK
        z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & MASK
        z ^= z >> 31
    return z


def draw_one(seed, b, k, n_units):
    """j(b, k), in Python integers of any size."""
    return (stream_first(seed, PURPOSE_DRAW, (b << 32) | k) * n_units) >> 64


def stream_first_array(seed, purpose, index):
    """stream_first for a uint64 array of indexes (uint64 arithmetic wraps like the device's)."""
    c = np.uint64
    with np.errstate(over="ignore"):
        z = (c(seed) * c(0x9e3779b97f4a7c15) + c(purpose) * c(0xaf251af3b0f025b5) + c(3) * c(0x9e3779b97f4a7c15)) + \
            index.astype(np.uint64) * c(0xd1342543de82ef95)
        z = (z ^ (z >> c(30))) * c(0xbf58476d1ce4e5b9)
        z = (z ^ (z >> c(27))) * c(0x94d049bb133111eb)
    return z ^ (z >> c(31))


def high_product(x, n_units):
    """(x * n_units) >> 64 for uint64 x and n_units <= 2^31, by 32-bit halves: x = h * 2^32 + l, so the product is
    h * U * 2^32 + l * U with both h * U and l * U below 2^63."""
    c = np.uint64
    high, low = x >> c(32), x & c(0xffffffff)
    return ((high * c(n_units) + ((low * c(n_units)) >> c(32))) >> c(32)).astype(np.int64)


def draws(seed, b, n_units):
    """int64[U]: j(b, 0) .. j(b, U - 1)."""
    index = (np.uint64(b) << np.uint64(32)) | np.arange(n_units, dtype=np.uint64)
    return high_product(stream_first_array(seed, PURPOSE_DRAW, index), n_units)


# ---- the table and the counts ------------------------------------------------------------------------------------------------
def unit_table(codes, unit, n_units):
    """int64[U][M][4]."""
    codes = np.asarray(codes, dtype=np.int64)
    n_sets, n = codes.shape
    unit = np.arange(n, dtype=np.int64) if unit is None else np.asarray(unit, dtype=np.int64)
    table = np.zeros((n_units, n_sets, 4), np.int64)
    for m in range(n_sets):
        np.add.at(table, (unit, m, codes[m]), 1)
    return table


def counts(codes, unit, n_units, n_boot, seed):
    """(counts int64[B][M][4], baseline int64[M][4])."""
    codes = np.asarray(codes)
    if codes.shape[1] == 0:
        return np.zeros((n_boot, codes.shape[0], 4), np.int64), np.zeros((codes.shape[0], 4), np.int64)
    table = unit_table(codes, unit, n_units)
    out = np.empty((n_boot,) + table.shape[1:], np.int64)
    for b in range(n_boot):
        out[b] = table[draws(seed, b, n_units)].sum(axis=0)
    return out, table.sum(axis=0)


def dense_units(groups):
    """Any 1-D array -> (int32 unit numbers in order of first appearance, how many)."""
    seen, unit = {}, []
    for value in np.asarray(groups).tolist():
        unit.append(seen.setdefault(value, len(seen)))
    return np.array(unit, np.int32), len(seen)


# ---- the statistics -----------------------------------------------------------------------------------------------------------
def errors(counts_, weight):
    counts_ = np.asarray(counts_, dtype=np.int64)
    return counts_[..., 2].astype(np.float64) + float(weight) * counts_[..., 1].astype(np.float64)


def interval(values, level):
    return np.quantile(np.asarray(values, np.float64), [(1 - level) / 2, (1 + level) / 2])


def standard_error(values):
    values = np.asarray(values, np.float64)
    return float(values.std(ddof=1)) if values.shape[0] > 1 else 0.0


def difference(errors_, a, b, level=0.95):
    d = errors_[:, a] - errors_[:, b]
    return dict(differences=d, mean=float(d.mean()), interval=tuple(float(v) for v in interval(d, level)),
                standard_error=standard_error(d),
                share_better=float((np.count_nonzero(d < 0) + 0.5 * np.count_nonzero(d == 0)) / d.shape[0]))


def model_codes(margins, target, threshold):
    """uint8 codes of float32 margins: 0 tn, 1 fp, 2 fn, 3 tp, with the float64 sigmoid of the exact margin (the device
    takes a float32 expf: `probability_gap` says how far the nearest probability is from the threshold), a NaN margin
    not positive."""
    wide = np.asarray(margins, np.float32).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        p = 1.0 / (1.0 + np.exp(-wide))
        positive = p > threshold
    actual = np.asarray(target) != 0
    return (2 * actual + positive).astype(np.uint8)


def probability_gap(margins, threshold):
    wide = np.asarray(margins, np.float32).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        p = 1.0 / (1.0 + np.exp(-wide))
    return float(np.nanmin(np.abs(p - threshold)))


def accuracy_codes(predicted, actual, not_found=-1):
    """0 correctly not found, 1 incorrectly matched, 2 incorrectly not found, 3 correctly matched."""
    out = []
    for p, a in zip(np.asarray(predicted).tolist(), np.asarray(actual).tolist()):
        out.append((3 if p == a else 1) if p != not_found else (0 if p == a else 2))
    return np.array(out, np.uint8)


# ---- the cases -----------------------------------------------------------------------------------------------------------------
# name: (n, U or None for rows as units, M, B, how the units are laid out, how the codes are drawn)
SHAPES = {
    "rows_1": (1, None, 1, 3, None, "random"),
    "rows_2": (2, None, 2, 5, None, "random"),
    "rows_63": (63, None, 2, 5, None, "random"),
    "rows_64": (64, None, 5, 5, None, "random"),
    "rows_65": (65, None, 1, 5, None, "random"),
    "rows_255": (255, None, 1, 9, None, "random"),
    "rows_256": (256, None, 2, 9, None, "random"),
    "rows_257": (257, None, 5, 9, None, "random"),
    "rows_m64": (65, None, 64, 3, None, "random"),
    "rows_b1": (100, None, 2, 1, None, "random"),
    "rows_two_chunks": (20000, None, 2, 2, None, "random"),    # 80,000 staged bytes, two chunks of draws
    "rows_chunks": (70001, None, 1, 2, None, "ones"),          # more draws of one class than a 16-bit field holds
    "rows_hbm": (40000, None, 5, 3, None, "random"),           # 8 staged bytes per row: 320,000 B
    "units_1": (50, 1, 2, 4, "random", "random"),
    "units_2": (31, 2, 2, 5, "random", "random"),
    "units_63": (150, 63, 2, 5, "random", "random"),
    "units_64": (90, 64, 5, 5, "random", "random"),
    "units_65": (200, 65, 1, 9, "random", "random"),
    "units_255": (400, 255, 1, 5, "random", "random"),
    "units_256": (300, 256, 2, 9, "random", "random"),
    "units_257": (700, 257, 5, 9, "random", "random"),
    "units_m64": (130, 65, 64, 3, "random", "random"),
    "units_b1": (100, 10, 2, 1, "random", "random"),
    "units_one_holds_all": (100, 7, 2, 5, "one", "random"),
    "units_overflow": (70002, 2, 1, 8, "1_and_rest", "ones"),  # two units of 1 and 70,001 rows, every code 1
    "units_hbm": (12000, 5000, 2, 3, "random", "random"),      # 16 B x 5000 x 2 = 160,000 B
}
NAMES = list(SHAPES)
SMALL = [name for name in NAMES if SHAPES[name][0] <= 1000]


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(codes uint8[M][n], unit int32[n] or None, n_units, n_boot, seed, counts, baseline): inputs drawn from the
    name's own seed, and the rule's answer."""
    n, n_units, n_sets, n_boot, layout, drawn = SHAPES[name]
    rng = np.random.RandomState(NAMES.index(name) + 100)
    codes = np.ones((n_sets, n), np.uint8) if drawn == "ones" else rng.randint(0, 4, (n_sets, n)).astype(np.uint8)
    if n_units is None:
        unit, n_units = None, n
    elif layout == "random":
        unit = rng.randint(0, n_units, n).astype(np.int32)
    elif layout == "one":
        unit = np.full(n, 3, np.int32)
    else:
        unit = np.ones(n, np.int32)
        unit[17] = 0
    seed = int(rng.randint(0, 1 << 31)) * 0x100000001 + NAMES.index(name)      # uses the high half of the seed too
    expected, baseline = counts(codes, unit, n_units, n_boot, seed)
    for array in (codes, unit, expected, baseline):
        if array is not None:
            array.setflags(write=False)
    return dict(name=name, codes=codes, unit=unit, n=n, n_units=n_units, n_sets=n_sets, n_boot=n_boot, seed=seed,
                counts=expected, baseline=baseline)


def unit_sizes(c):
    return np.ones(c["n"], np.int64) if c["unit"] is None else np.bincount(c["unit"], minlength=c["n_units"])


def table_bytes(c):
    """What the kernel would stage: 16 bytes per unit and set with units, one byte per row and set (the sets padded to
    a multiple of four) without."""
    return 16 * c["n_units"] * c["n_sets"] if c["unit"] is not None else c["n_units"] * ((c["n_sets"] + 3) // 4 * 4)
