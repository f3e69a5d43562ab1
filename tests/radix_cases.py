"""Float32 columns whose radix-sort keys differ in chosen bytes, for the consumers of radix_sort_columns
(csrc/ds_radix.h): the cuts, the AUC and the isotonic calibration.  The sort skips the pass of a byte that is the same in
every key of a column, per column, and every consumer recomputes the buffer the column ends in from the passes done; a
4-bit MASK names the bytes that differ (bit p: byte p, the digit of pass p), so the 16 masks are the 16 skip patterns.

Everything is generated from seeds by the code below; nothing here calls the code under test.  The families at the end
are what tests/test_gpu_radix_consumers.py runs, with what each column is meant to be; tests/test_radix_cases_cpu.py
proves those statements with its own restatement of the key."""
import numpy as np

BASE_BITS = 0x3F123456          # 0.571...: finite and positive, so key = bits ^ 0x80000000
MASKS = tuple(range(16))
TILE = 8192                     # kSortTile
ALL_BYTES = 15


def _f32(values):
    return np.ascontiguousarray(values, dtype=np.float32)


def masked_column(mask, n, seed):
    """float32[n], n >= 2, whose keys differ in exactly the bytes of `mask`: bits 0x3F123456 in every row; byte p < 3 of
    a set bit holds random values with 0x00 in row 0 and 0xFF in row n - 1; byte 3 holds random values in [0x30, 0x50)
    with 0x3F and 0x40 in those rows.  All values are finite and positive."""
    assert 0 <= mask < 16 and n >= 2
    rng = np.random.default_rng(seed)
    bits = np.full(n, BASE_BITS, np.uint32)
    for p in range(4):
        if not (mask >> p) & 1:
            continue
        if p == 3:
            byte = rng.integers(0x30, 0x50, n).astype(np.uint32)
            byte[0], byte[-1] = 0x3F, 0x40
        else:
            byte = rng.integers(0, 256, n).astype(np.uint32)
            byte[0], byte[-1] = 0x00, 0xFF
        bits = (bits & ~np.uint32(0xFF << (8 * p))) | (byte << np.uint32(8 * p))
    return bits.view(np.float32)


def few(mask, n, distinct, seed):
    """masked_column's values drawn from at most `distinct` different ones (the two planted rows among them), so that a
    consumer that reads the heads of the sorted column reads every one of them."""
    assert 2 <= distinct <= n
    pool = masked_column(mask, distinct, seed)
    column = pool[np.random.default_rng(seed + 7919).integers(0, distinct, n)]
    column[0], column[-1] = pool[0], pool[-1]
    return _f32(column)


def with_nans(column, share, seed):
    """A copy with about `share` of the rows NaN; rows 0 and n - 1 (the planted bytes) stay."""
    out = _f32(column).copy()
    drop = np.random.default_rng(seed + 104729).random(out.shape[0]) < share
    drop[0] = drop[-1] = False
    out[drop] = np.nan
    return out


def mixed_signs(column, seed):
    """A copy with about half of the rows negated (row 0 stays, row n - 1 is negated): the key of a negative value is
    the complement of its bits, so every byte differs between the two signs and no pass is skipped."""
    out = _f32(column).copy()
    flip = np.random.default_rng(seed + 1299709).random(out.shape[0]) < 0.5
    flip[0], flip[-1] = False, True
    out[flip] = -out[flip]
    return out


# ---- calibration: two columns (negatives, positives) of one fit ----------------------------------------------------------
SMALL_NEG, SMALL_POS = 300, 211
LARGE_NEG, LARGE_POS = 2 * TILE + 5, TILE + 1
SMALL_PAIRS = tuple((a, b) for a in MASKS for b in MASKS)
LARGE_PAIRS = tuple((a, (7 * a + 3) % 16) for a in MASKS)      # 7 is odd: the positives' masks are a permutation
NAN_SHARE = 0.01


def calibration_case(mask_neg, mask_pos, n_neg, n_pos, nan_share=0.0):
    """(scores, target) float32[n_neg + n_pos], rows shuffled: negatives masked_column(mask_neg), positives
    masked_column(mask_pos) around the same bits (equal masks share keys: ties between the columns).  Both of the fit's
    columns have the length n_neg + n_pos, so each is padded by the other's length.  NaN rows are dropped by the fit
    and stay out of the OR / AND: the masks hold with them."""
    neg, pos = masked_column(mask_neg, n_neg, mask_neg), masked_column(mask_pos, n_pos, 100 + mask_pos)
    if nan_share:
        neg, pos = with_nans(neg, nan_share, mask_neg), with_nans(pos, nan_share, 100 + mask_pos)
    scores = np.concatenate([neg, pos])
    target = np.concatenate([np.zeros(n_neg, np.float32), np.ones(n_pos, np.float32)])
    order = np.random.default_rng(1000 + 16 * mask_neg + mask_pos).permutation(n_neg + n_pos)
    return _f32(scores[order]), _f32(target[order])


def calibration_families():
    """family -> list of (name, mask_neg, mask_pos, n_neg, n_pos, nan_share)."""
    return {
        "small": [(f"{a:04b}-{b:04b}", a, b, SMALL_NEG, SMALL_POS, 0.0) for a, b in SMALL_PAIRS],
        "large": [(f"{a:04b}-{b:04b}", a, b, LARGE_NEG, LARGE_POS, 0.0) for a, b in LARGE_PAIRS],
        "large_nan": [(f"{a:04b}-{b:04b}", a, b, LARGE_NEG, LARGE_POS, NAN_SHARE) for a, b in LARGE_PAIRS],
    }


# ---- AUC: one column, the negatives ----------------------------------------------------------------------------------------
AUC_NEGATIVES = (257, TILE + 1, 2 * TILE + 5)
AUC_POSITIVES = 1000
AUC_NAN_MASK = 0b0101          # the variant with a NaN negative is built on this column


def auc_case(mask, n_neg, nan_negative=False):
    """(scores, labels), rows shuffled.  Negatives: masked_column(mask, n_neg); with nan_negative one of them (not a
    planted row) is a NaN, whose key 0xFFFFFFFF is the padding's and counts in the OR / AND.  1000 positives: 332 of
    the negatives' own values (ties), 332 float32 neighbours above and 330 below such values, and -inf, +inf, 0.0,
    -0.0 and two NaNs."""
    rng = np.random.default_rng(5000 + 16 * n_neg + mask)
    neg = masked_column(mask, n_neg, mask)
    own = neg[rng.integers(0, n_neg, 332)]
    above = np.nextafter(neg[rng.integers(0, n_neg, 332)], np.float32(np.inf))
    below = np.nextafter(neg[rng.integers(0, n_neg, 330)], np.float32(-np.inf))
    special = _f32([-np.inf, np.inf, 0.0, -0.0, np.nan, -np.nan])
    pos = np.concatenate([own, above, below, special]).astype(np.float32)
    assert pos.shape[0] == AUC_POSITIVES
    if nan_negative:
        neg = neg.copy()
        neg[n_neg // 2] = np.nan
    scores = np.concatenate([neg, pos])
    labels = np.concatenate([np.zeros(n_neg, np.float32), np.ones(pos.shape[0], np.float32)])
    order = rng.permutation(scores.shape[0])
    return _f32(scores[order]), _f32(labels[order])


def auc_family(n_neg):
    """list of (name, mask, nan_negative, the mask the device sees)."""
    return [(f"{mask:04b}", mask, False, mask) for mask in MASKS] + [(f"{AUC_NAN_MASK:04b}-nan", AUC_NAN_MASK, True, ALL_BYTES)]


# ---- cuts: many columns of one launch ----------------------------------------------------------------------------------------
CUT_ROWS = (TILE + 1, 2 * TILE + 5)
FEW_DISTINCT = 200             # below max_bin - 1 = 255: every head of the sorted column becomes a cut
CUT_NAN_SHARE = 0.3


def cuts_matrix(n):
    """(float32[n, 80], columns): 16 masked_columns, 16 few(mask, n, 200), the same 32 with 30 % NaN and 16 mixed-sign
    copies.  columns[f] = (name, the mask the device sees, the largest number of distinct non-NaN keys or None).  In the
    cuts a NaN's key counts in the OR / AND, so a column with NaNs skips no pass; nor does one with both signs."""
    data, columns = [], []
    for mask in MASKS:
        data.append(masked_column(mask, n, 200 + mask))
        columns.append((f"masked_{mask:04b}", mask, None))
    for mask in MASKS:
        data.append(few(mask, n, FEW_DISTINCT, 300 + mask))
        columns.append((f"few_{mask:04b}", mask, FEW_DISTINCT))
    for f in range(32):
        data.append(with_nans(data[f], CUT_NAN_SHARE, 400 + f))
        columns.append((columns[f][0] + "_nan", ALL_BYTES, columns[f][2]))
    for mask in MASKS:
        data.append(mixed_signs(data[mask], 500 + mask))
        columns.append((f"mixed_{mask:04b}", ALL_BYTES, None))
    return np.ascontiguousarray(np.column_stack(data), dtype=np.float32), columns
