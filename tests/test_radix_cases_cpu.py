"""The columns of tests/radix_cases.py are what their names say, proved without the library: cut_key of csrc/ds_radix.h
is restated here in NumPy, and for every case that tests/test_gpu_radix_consumers.py runs the bytes in which the keys
of a column differ (as the consumer in question forms its OR / AND), the parity of the passes that then run (the buffer
the column ends in) and the number of distinct keys are computed from the data.  Every family holds all 16 skip
patterns and both parities."""
import numpy as np
import pytest

import radix_cases as cases


def cut_key(values):
    """ds_radix.h: 0xFFFFFFFF for a NaN; else, with -0.0 read as +0.0, all bits flipped under a set sign bit and only
    the sign bit flipped otherwise."""
    bits = np.ascontiguousarray(values, dtype=np.float32).view(np.uint32).copy()
    nan = (bits & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    bits[bits == np.uint32(0x80000000)] = 0
    key = np.where(bits & np.uint32(0x80000000), ~bits, bits ^ np.uint32(0x80000000)).astype(np.uint32)
    key[nan] = 0xFFFFFFFF
    return key


def differing_mask(keys):
    """bit p set iff byte p of (OR ^ AND) of the keys is not zero: pass p runs."""
    differing = int(np.bitwise_or.reduce(keys) ^ np.bitwise_and.reduce(keys)) if keys.shape[0] else 0xFFFFFFFF
    return sum(1 << p for p in range(4) if (differing >> (8 * p)) & 0xFF)


def parity(mask):
    return bin(mask).count("1") & 1            # passes_done(differing, 4) & 1: odd -> the column ends in keys_b


def covers_every_pattern(masks):
    masks = set(masks)
    return masks >= set(cases.MASKS) and {parity(m) for m in masks} == {0, 1}


def test_the_key_restated_here_orders_floats_and_sends_nan_last():
    values = np.float32([-np.inf, -3.5, -1e-45, -0.0, 0.0, 1e-45, 0.571, 1.0, np.inf, np.nan])
    keys = cut_key(values)
    assert keys[3] == keys[4] == 0x80000000 and keys[-1] == 0xFFFFFFFF
    assert (np.diff(keys[[0, 1, 2, 3, 5, 6, 7, 8, 9]].astype(np.int64)) > 0).all()
    assert cut_key(np.uint32([cases.BASE_BITS]).view(np.float32))[0] == cases.BASE_BITS ^ 0x80000000


@pytest.mark.parametrize("n", [2, 300, 2 * cases.TILE + 5])
def test_masked_column_differs_in_exactly_the_bytes_of_its_mask(n):
    for mask in cases.MASKS:
        column = cases.masked_column(mask, n, mask)
        assert column.dtype == np.float32 and column.shape == (n,)
        assert np.isfinite(column).all() and (column > 0).all()
        keys = cut_key(column)
        assert np.array_equal(keys, column.view(np.uint32) ^ np.uint32(0x80000000))
        assert differing_mask(keys) == mask, (n, mask)
        assert cases.masked_column(mask, n, mask).tobytes() == column.tobytes()       # a function of its arguments


def test_few_and_with_nans_keep_the_mask():
    for mask in cases.MASKS:
        for n in (300, cases.TILE + 1):
            column = cases.few(mask, n, cases.FEW_DISTINCT, mask)
            keys = cut_key(column)
            assert differing_mask(keys) == mask and np.unique(keys).shape[0] <= cases.FEW_DISTINCT
            assert np.unique(keys).shape[0] >= (2 if mask else 1)
            holed = cases.with_nans(column, 0.3, mask)
            kept = ~np.isnan(holed)
            assert 0.2 * n < np.count_nonzero(~kept) < 0.4 * n
            assert np.array_equal(holed[kept].view(np.uint32), column[kept].view(np.uint32))
            assert differing_mask(cut_key(holed[kept])) == mask


@pytest.mark.parametrize("family", sorted(cases.calibration_families()))
def test_calibration_columns(family):
    """The fit's columns are the keys of the rows of a label without the NaN rows; the padding is in neither OR / AND."""
    seen_neg, seen_pos, seen_pairs = [], [], set()
    for name, mask_neg, mask_pos, n_neg, n_pos, nan_share in cases.calibration_families()[family]:
        scores, target = cases.calibration_case(mask_neg, mask_pos, n_neg, n_pos, nan_share)
        assert scores.shape == target.shape == (n_neg + n_pos,) and set(np.unique(target)) == {0.0, 1.0}
        keys = cut_key(scores)
        kept = keys != 0xFFFFFFFF
        assert (np.count_nonzero(~kept) > 0) == (nan_share > 0), name
        negatives, positives = keys[kept & (target == 0)], keys[kept & (target != 0)]
        assert negatives.shape[0] + np.count_nonzero(~kept & (target == 0)) == n_neg
        assert differing_mask(negatives) == mask_neg and differing_mask(positives) == mask_pos, name
        # more than a tile of padding behind each column of the large fits
        if family != "small":
            assert scores.shape[0] - negatives.shape[0] > cases.TILE and scores.shape[0] - positives.shape[0] > cases.TILE
            assert negatives.shape[0] > 2 * cases.TILE - 0.02 * n_neg and positives.shape[0] > cases.TILE - 0.02 * n_pos
        if mask_neg == mask_pos and mask_neg in (0, 1):   # at most 256 keys around the same bits: the columns share keys
            assert np.intersect1d(negatives, positives).shape[0] > 0, name
        seen_neg.append(mask_neg)
        seen_pos.append(mask_pos)
        seen_pairs.add((parity(mask_neg), parity(mask_pos)))
    assert covers_every_pattern(seen_neg) and covers_every_pattern(seen_pos)
    assert seen_pairs == {(0, 0), (0, 1), (1, 0), (1, 1)}       # the two columns end in the same and in different buffers
    if family == "small":
        assert len(set(zip(seen_neg, seen_pos))) == 256


@pytest.mark.parametrize("n_neg", cases.AUC_NEGATIVES)
def test_auc_columns(n_neg):
    """The metrics' column is the keys of ALL negatives: a NaN negative counts in the OR / AND."""
    seen = []
    for name, mask, nan_negative, device_mask in cases.auc_family(n_neg):
        scores, labels = cases.auc_case(mask, n_neg, nan_negative)
        keys = cut_key(scores)
        negatives, positives = keys[labels == 0], keys[labels != 0]
        assert negatives.shape[0] == n_neg and positives.shape[0] == cases.AUC_POSITIVES
        assert differing_mask(negatives) == device_mask, name
        assert np.count_nonzero(negatives == 0xFFFFFFFF) == int(nan_negative)
        assert np.count_nonzero(positives == 0xFFFFFFFF) == 2
        real = negatives[negatives != 0xFFFFFFFF]
        assert differing_mask(real) == mask
        ties = np.isin(positives, real)
        assert np.count_nonzero(ties) >= 330 and np.count_nonzero(~ties) >= 6
        if not nan_negative:
            seen.append(device_mask)
    assert covers_every_pattern(seen)
    assert [case[3] for case in cases.auc_family(n_neg) if case[2]] == [cases.ALL_BYTES]


@pytest.mark.parametrize("n", cases.CUT_ROWS)
def test_cut_columns(n):
    """The cuts' column is the keys of all rows, NaNs included."""
    x, columns = cases.cuts_matrix(n)
    assert x.shape == (n, 80) == (n, len(columns)) and x.dtype == np.float32
    assert len({name for name, _, _ in columns}) == 80
    seen, kinds = [], {}
    for f, (name, device_mask, distinct) in enumerate(columns):
        keys = cut_key(x[:, f])
        assert differing_mask(keys) == device_mask, name
        real = np.unique(keys[keys != 0xFFFFFFFF])
        if distinct is not None:
            assert real.shape[0] <= distinct < 255, name         # at most max_bin - 1 heads at max_bin 256: all are cuts
        if name.endswith("_nan"):
            assert 0.2 * n < np.count_nonzero(keys == 0xFFFFFFFF) < 0.4 * n
        elif name.startswith("mixed_"):
            assert 0.4 * n < np.count_nonzero(x[:, f] < 0) < 0.6 * n
        else:
            seen.append(device_mask)
        kinds.setdefault(name.split("_")[0] + ("_nan" if name.endswith("_nan") else ""), []).append(device_mask)
    assert {kind: len(masks) for kind, masks in kinds.items()} == {"masked": 16, "few": 16, "masked_nan": 16,
                                                                   "few_nan": 16, "mixed": 16}
    assert covers_every_pattern(kinds["masked"]) and covers_every_pattern(kinds["few"])
    assert set(kinds["masked_nan"] + kinds["few_nan"] + kinds["mixed"]) == {cases.ALL_BYTES}
    # columns of different parity are neighbours in every grouping the GPU test runs (groups of 1, 5, 80 columns)
    parities = [parity(mask) for _, mask, _ in columns[:32]]
    assert any(parities[f] != parities[f + 1] for f in range(31))
