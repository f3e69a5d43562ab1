"""compute_cuts_device (csrc/ds_cuts.hip) against the two host statements of the cut rule, train.compute_cuts and
tests/forest_train_oracle.cuts, bit for bit: make_data matrices up to 1.2M rows, crafted columns at the boundaries of
the rule, the real construct_features matrix, every column grouping, repeated calls, and untouched neighbours of the
outputs."""
import ctypes

import numpy as np
import pytest

import cuts_cases
import forest_train_oracle as oracle
from cuts_cases import same_bits
from forest_train_oracle import make_data

pytestmark = pytest.mark.gpu


def expected_cuts(x, max_bin):
    """(cuts, offsets) of compute_cuts, checked equal to the oracle's."""
    import doppel_speller_amd as ds
    cuts, offsets = ds.compute_cuts(x, max_bin)
    per_feature = oracle.cuts(x, max_bin)
    assert same_bits(cuts, np.concatenate(per_feature).astype(np.float32))
    assert offsets.tolist() == [0] + np.cumsum([c.size for c in per_feature]).tolist()
    return cuts, offsets


def device_cuts(x, max_bin):
    import doppel_speller_amd as ds
    from doppel_speller_amd import _lib
    d_x = _lib.DeviceArray.from_host(x)
    try:
        return ds.compute_cuts_device(d_x, x.shape[0], max_bin)
    finally:
        d_x.free()


def check(x, max_bin, names=None):
    cuts, offsets = device_cuts(x, max_bin)
    want, want_offsets = expected_cuts(x, max_bin)
    assert offsets.dtype == np.int32 and cuts.dtype == np.float32
    if offsets.tolist() != want_offsets.tolist() or not same_bits(cuts, want):
        for f in range(x.shape[1]):
            got_f, want_f = cuts[offsets[f]:offsets[f + 1]], want[want_offsets[f]:want_offsets[f + 1]]
            assert same_bits(got_f, want_f), (names[f] if names else f, max_bin, got_f[:8], want_f[:8])
    return cuts, offsets


@pytest.mark.parametrize("max_bin", [256, 16, 2])
@pytest.mark.parametrize("n, nf", [(1, 3), (5003, 66), (100000, 96), (1200000, 12)])
def test_make_data_matrices(n, nf, max_bin):
    x, _ = make_data(n, nf, n + nf)
    check(x, max_bin)


@pytest.mark.parametrize("max_bin", [256, 16, 2])
def test_crafted_columns(max_bin):
    x, names = cuts_cases.crafted_matrix()
    cuts, offsets = check(x, max_bin, names)
    counts = dict(zip(names, np.diff(offsets).tolist()))
    assert counts["all_nan"] == 0 and counts["one_value"] == 0 and counts["all_equal"] == 0
    if max_bin == 256:
        assert counts["distinct_254"] == 253 and counts["distinct_255"] == 254 and counts["distinct_256"] <= 254
        assert counts["distinct_255_nan_30"] == 254 and counts["signed_zeros"] == 2


def test_crafted_columns_one_by_one_and_in_any_company():
    """A column's cuts do not depend on its neighbours or its place (columns ride in blockIdx.y)."""
    x, names = cuts_cases.crafted_matrix(seed=3)
    whole, offsets = check(x, 256, names)
    order = np.random.RandomState(1).permutation(x.shape[1])
    shuffled, shuffled_offsets = device_cuts(np.ascontiguousarray(x[:, order]), 256)
    for place, f in enumerate(order):
        alone, _ = device_cuts(np.ascontiguousarray(x[:, f:f + 1]), 256)
        want = whole[offsets[f]:offsets[f + 1]]
        assert same_bits(alone, want), names[f]
        assert same_bits(shuffled[shuffled_offsets[place]:shuffled_offsets[place + 1]], want), names[f]


def test_rows_beyond_one_sort_tile_and_one_row_short_of_it():
    """Row counts around the 8192-key sort tile and the 64-row key tile."""
    for n in (63, 64, 65, 8191, 8192, 8193, 3 * 8192 + 1):
        x, _ = make_data(n, 7, n)
        check(x, 256)
        check(x, 16)


@pytest.fixture(scope="module")
def real_features():
    """construct_features of the 20k x 4k synthetic training set (tests/test_gpu_training_set.py), made by the host
    path."""
    import doppel_speller_amd as ds
    from doppel_speller_amd import synth
    w = synth.make_workload(20000, 4000, seed=21, query_seed=22)
    truth = synth._to_strings(w.t_flat, w.t_off)
    train = synth._to_strings(w.q_flat, w.q_off)
    ids = np.where(w.actual_row >= 0, w.title_id[np.maximum(w.actual_row, 0)], -1)
    fe = ds.FeatureEngineering(truth, w.title_id, train, ids, seed=9, transform=False)
    fe.generate_train_and_evaluation_data_sets()
    return fe.features


@pytest.mark.parametrize("max_bin", [256, 16, 2])
def test_real_feature_matrix(real_features, max_bin):
    assert real_features.shape[1] == 66 and real_features.shape[0] > 50000 and np.isnan(real_features).any()
    check(real_features, max_bin)


def test_two_calls_give_identical_bytes(real_features):
    first, second = device_cuts(real_features, 256), device_cuts(real_features, 256)
    assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()


def test_result_does_not_depend_on_the_column_group(real_features):
    from doppel_speller_amd.train import cuts_option
    crafted, _ = cuts_cases.crafted_matrix()
    wide, _ = make_data(20000, 96, 5)
    try:
        for x in (real_features, crafted, wide):
            results = []
            for group in (0, 1, 5, x.shape[1]):
                cuts_option("column_group", group)
                results.append(device_cuts(x, 256))
            want = expected_cuts(x, 256)
            for cuts, offsets in results:
                assert same_bits(cuts, want[0]) and offsets.tolist() == want[1].tolist()
    finally:
        cuts_option("column_group", 0)


def test_neighbours_of_the_outputs_and_the_input_stay_untouched():
    from doppel_speller_amd import _lib
    x, _ = make_data(5003, 66, 3)
    n, nf = x.shape
    pad = 4096
    want, want_offsets = expected_cuts(x, 256)
    total = want.shape[0]
    cuts = np.full(pad + nf * 254 + pad, -12345.0, np.float32)
    offsets = np.full(pad + nf + 1 + pad, -777, np.int32)
    sentinel = np.float32(3.25)
    staged = np.full(pad + n * nf + pad, sentinel, np.float32)
    staged[pad:pad + n * nf] = x.reshape(-1)
    d_staged = _lib.DeviceArray.from_host(staged)
    address = d_staged.ptr.value + 4 * pad
    _lib.check(_lib.lib().ds_feature_cuts_device(ctypes.c_void_p(address), n, nf, 256,
                                                 ctypes.c_void_p(cuts.ctypes.data + 4 * pad),
                                                 ctypes.c_void_p(offsets.ctypes.data + 4 * pad), 0, None),
               "ds_feature_cuts_device")
    assert same_bits(cuts[pad:pad + total], want)
    assert (cuts[:pad] == -12345.0).all() and (cuts[pad + total:] == -12345.0).all()   # nothing past the last cut
    assert offsets[pad:pad + nf + 1].tolist() == want_offsets.tolist()
    assert (offsets[:pad] == -777).all() and (offsets[pad + nf + 1:] == -777).all()
    assert d_staged.to_host().tobytes() == staged.tobytes()


def test_a_stream_of_the_callers(real_features):
    import doppel_speller_amd as ds
    from doppel_speller_amd import _lib
    stream = ctypes.c_void_p()
    _lib.check(_lib.lib().ds_stream_create(0, ctypes.byref(stream)), "ds_stream_create")
    try:
        x = real_features[:30000]
        d_x = _lib.DeviceArray.from_host(x)
        cuts, offsets = ds.compute_cuts_device(d_x, x.shape[0], 256, stream=stream)
        want = expected_cuts(x, 256)
        assert same_bits(cuts, want[0]) and offsets.tolist() == want[1].tolist()
        fewer, _ = ds.compute_cuts_device(d_x, 1000, 256, stream=stream)      # the first n rows of a larger matrix
        assert same_bits(fewer, expected_cuts(x[:1000], 256)[0])
    finally:
        _lib.lib().ds_stream_destroy(stream, 0)
