"""The trainer's contract without a GPU: the oracle's cuts and bin rule, split choice on hand-worked histograms,
fit's argument checks and the C entry points' argument errors."""
import ctypes
import os

import numpy as np
import pytest

import forest_train_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def check_bin_rule(column, c):
    b = oracle.bins(np.asarray(column, np.float32)[:, None], [c])[0]
    x = np.asarray(column, np.float32)
    assert (b[np.isnan(x)] == 255).all()
    for k in range(1, c.size + 1):                  # bin(x) < b  <=>  x < cuts[b - 1], for every cut
        present = ~np.isnan(x)
        assert np.array_equal((b[present] < k), (x[present] < c[k - 1]))


def test_cuts_and_bins_on_crafted_columns():
    inf = np.float32(np.inf)
    column = np.array([np.nan, -0.0, 0.0, 1.5, -inf, inf, 1.5, np.nan, -2.0], np.float32)
    c = oracle.cuts_of(column)
    assert c.tolist() == [-2.0, 0.0, 1.5, np.inf]     # distinct without the smallest (-inf)
    assert not np.signbit(c[1])                       # -0.0 counts as +0.0
    assert oracle.bins(column[:, None], [c])[0].tolist() == [255, 2, 2, 3, 0, 4, 3, 255, 1]
    check_bin_rule(column, c)
    assert oracle.cuts_of(np.full(10, 3.0, np.float32)).size == 0                 # constant feature
    assert oracle.cuts_of(np.full(10, np.nan, np.float32)).size == 0              # all-NaN feature
    assert oracle.bins(np.full((4, 1), np.nan, np.float32), [np.zeros(0, np.float32)])[0].tolist() == [255] * 4


@pytest.mark.parametrize("distinct", [255, 256, 1000])
def test_cuts_at_the_distinct_value_limit(distinct):
    rng = np.random.RandomState(distinct)
    values = (np.arange(distinct, dtype=np.float32) * np.float32(0.25)) - 7
    column = rng.choice(values, 5000).astype(np.float32)
    column[:distinct] = values                         # every value present
    c = oracle.cuts_of(column)
    if distinct <= 255:
        assert np.array_equal(c, values[1:])
    else:
        v = np.sort(column)
        expected = np.unique(v[(np.arange(1, 255) * v.size) // 255])
        assert np.array_equal(c, expected[expected != v[0]]) and c.size <= 254
    check_bin_rule(column, c)
    assert oracle.bins(column[:, None], [c]).max() <= 254


def test_product_cuts_equal_the_oracle():
    from doppel_speller_amd.train import compute_cuts
    rng = np.random.RandomState(3)
    features = rng.randn(3000, 7).astype(np.float32)
    features[:, 1] = np.round(features[:, 1] * 3)       # few distinct values
    features[::7, 2] = np.nan
    features[:, 3] = -0.0
    features[:5, 3] = 0.0
    features[:, 4] = np.nan
    features[:, 5] = rng.randint(0, 255, 3000)           # exactly 255 distinct values
    features[:, 6] = rng.randint(0, 256, 3000)           # 256 distinct values: quantile cuts
    for max_bin in (256, 16):
        cuts, offsets = compute_cuts(features, max_bin)
        for f, expected in enumerate(oracle.cuts(features, max_bin)):
            got = cuts[offsets[f]:offsets[f + 1]]
            assert np.array_equal(got.view(np.uint32), expected.view(np.uint32)), (max_bin, f)


def hist_of(per_feature_bins):
    """int64[nf, 256, 2] from {feature: {bin: (qg, qh)}} in units of 2^-30."""
    nf = len(per_feature_bins)
    hist = np.zeros((nf, 256, 2), np.int64)
    for f, entries in enumerate(per_feature_bins):
        for b, (g, h) in entries.items():
            hist[f, b] = (g, h)
    return hist


Q = 1 << 30


def test_split_choice_hand_worked():
    # one feature, bins 0..2 (2 cuts): G = (-2, 2, 0) H = (1, 1, 2)
    hist = hist_of([{0: (-2 * Q, Q), 1: (2 * Q, Q), 2: (0, 2 * Q)}])
    gain, f, b, missing_left, (lg, lh) = oracle.best_split(hist, [2], reg_lambda=1.0, min_child_weight=0.0)
    # b = 1: left (-2, 1), right (2, 3): 4/2 + 4/4 - 0/5 = 3;  b = 2: left (0, 2), right (0, 2): 0
    assert (f, b, missing_left, lg, lh) == (0, 1, 0, -2 * Q, Q) and gain == 3.0
    # min_child_weight 1.5 rejects b = 1 (HL = 1): only b = 2 remains, with gain 0
    gain, f, b, missing_left, _ = oracle.best_split(hist, [2], reg_lambda=1.0, min_child_weight=1.5)
    assert (b, gain) == (2, 0.0)
    assert oracle.best_split(hist, [2], reg_lambda=1.0, min_child_weight=2.5) is None
    assert oracle.best_split(hist, [0], reg_lambda=1.0, min_child_weight=0.0) is None   # no cuts, no candidates


def test_split_ties_and_missing_direction():
    same = {0: (-2 * Q, Q), 1: (2 * Q, Q)}
    # two identical features: the lower feature wins
    _, f, b, missing_left, _ = oracle.best_split(hist_of([same, same]), [1, 1], 1.0, 0.0)
    assert (f, b, missing_left) == (0, 1, 0)
    # no missing values: right and left give the same gain, missing right wins
    _, _, _, missing_left, _ = oracle.best_split(hist_of([same]), [1], 1.0, 0.0)
    assert missing_left == 0
    # missing rows with a negative gradient join the negative side: left
    with_missing = {0: (-2 * Q, Q), 1: (2 * Q, Q), 255: (-3 * Q, Q)}
    gain, _, b, missing_left, (lg, lh) = oracle.best_split(hist_of([with_missing]), [1], 1.0, 0.0)
    assert (b, missing_left, lg, lh) == (1, 1, -5 * Q, 2 * Q)
    assert gain == 25 / 3 + 4 / 2 - 9 / 4
    # equal gain at b = 1 and b = 3 of one feature: the lower b
    # b = 1: L (-1, 1) R (1, 3) and b = 3: L (-1, 3) R (1, 1) both gain 1/2 + 1/4; b = 2 gains 0
    sym = hist_of([{0: (-Q, Q), 1: (Q, Q), 2: (-Q, Q), 3: (Q, Q)}])
    gain, _, b, _, _ = oracle.best_split(sym, [3], 1.0, 0.0)
    assert (b, gain) == (1, 0.75)
    tie = hist_of([{0: (-Q, Q), 1: (Q, Q)}, {0: (Q, Q), 1: (-Q, Q)}])
    _, f, _, _, _ = oracle.best_split(tie, [1, 1], 1.0, 0.0)
    assert f == 0


def test_grow_tree_by_hand():
    # 4 rows, one feature with bins 0, 0, 1, 1 and gradients -1, -1, +1, +1 (hessian 1): one split, two leaves
    node_bins = np.array([[0, 0, 1, 1]], np.uint8)
    gh = np.array([[-Q, Q], [-Q, Q], [Q, Q], [Q, Q]], np.int64)
    tree, leaves = oracle.grow_tree(node_bins, [1], gh, max_depth=3, eta=0.5, min_child_weight=1.0, reg_lambda=1.0)
    assert tree["state"][:3].tolist() == [2, 3, 3] and tree["bin"][0] == 1
    assert tree["leaf"][1] == np.float32(2 / 3 * 0.5) and tree["leaf"][2] == np.float32(-2 / 3 * 0.5)
    assert leaves.tolist() == [tree["leaf"][1]] * 2 + [tree["leaf"][2]] * 2


def test_gradients_rule():
    p = np.array([0.5, 0.25, 0.999], np.float32)
    y = np.array([1, 0, 0], np.float32)
    gh = oracle.gradients(p, y, 5.0)
    assert gh[0].tolist() == [-Q // 2, Q // 4]                    # w = 1: g = -0.5, h = 0.25
    assert gh[1].tolist() == [int(np.rint(1.25 * Q)), int(np.rint(0.25 * 0.75 * 5 * Q))]


def test_fit_argument_validation():
    import doppel_speller_amd as ds
    from doppel_speller_amd.train import validate_fit
    x = np.zeros((10, 3), np.float32)
    y = np.zeros(10)
    trainer = ds.ForestTrainer()
    bad = [
        (np.zeros(10, np.float32), y, {}),                    # 1-D features
        (np.zeros((0, 3), np.float32), np.zeros(0), {}),       # no rows
        (np.zeros((10, 97), np.float32), y, {}),               # more than 96 features
        (x, np.zeros(9), {}),                                  # label count
        (x, np.full(10, 2.0), {}),                             # labels outside {0, 1}
        (x, y, dict(eval_features=np.zeros((4, 2), np.float32), eval_target=np.zeros(4))),   # columns differ
        (x, y, dict(eval_features=np.zeros((4, 3), np.float32))),                            # target missing
        (x, y, dict(max_depth=0)), (x, y, dict(max_depth=9)), (x, y, dict(eta=0)), (x, y, dict(eta=float("nan"))),
        (x, y, dict(min_child_weight=-1)), (x, y, dict(reg_lambda=0, min_child_weight=0)),
        (x, y, dict(num_boost_round=0)), (x, y, dict(early_stopping_rounds=True)), (x, y, dict(max_bin=1)),
        (x, y, dict(max_bin=257)), (x, y, dict(beta=0)),
    ]
    for features, target, extra in bad:
        with pytest.raises(ValueError):
            validate_fit(features, target, **extra)
        with pytest.raises(ValueError):                        # fit checks before any library call
            trainer.fit(features, target, **extra)
    out = validate_fit(x, y.astype(np.int64))
    assert out[0].dtype == np.float32 and out[1].dtype == np.float32 and out[2] is None


def test_feature_importance_and_save_format(tmp_path):
    pytest.importorskip("numpy")
    from doppel_speller_amd.forest import ForestModel
    model = ForestModel.__new__(ForestModel)                    # host-only parts: no device handle
    model.arrays = dict(feature=np.array([1, -1, 1, 0, -1, -1, -1], np.int32))
    model.n_features = 3
    assert model.feature_importance().tolist() == [1 / 3, 2 / 3, 0.0]
    model.arrays = dict(feature=np.array([-1], np.int32))
    assert model.feature_importance().tolist() == [0.0, 0.0, 0.0]


@pytest.fixture(scope="module")
def library():
    path = os.path.join(ROOT, "doppel-speller_amd", "libdoppel_amd.so")
    if not os.path.exists(path):
        pytest.skip("library not built")
    handle = ctypes.CDLL(path)
    handle.ds_last_error.restype = ctypes.c_char_p
    return handle


def test_trainer_entry_points_reject_bad_arguments(library):
    p = ctypes.c_void_p
    d = ctypes.c_double
    out = p()
    features = np.zeros((4, 2), np.float32)
    cuts = np.array([0.5, 0.25], np.float32)
    good_offsets = np.array([0, 1, 1], np.int32)

    def create(feat=features, n=4, nf=2, c=cuts, offsets=good_offsets, depth=5, eta=0.1, mcw=1.0, lam=1.0, beta=5.0):
        ptr = lambda a: None if a is None else a.ctypes.data_as(p)
        return library.ds_trainer_create(ptr(feat), ctypes.c_int64(n), ctypes.c_int32(nf), ptr(c), ptr(offsets),
                                         ctypes.c_int32(depth), d(eta), d(mcw), d(lam), d(beta), 0, ctypes.byref(out))

    assert library.ds_trainer_create(None, ctypes.c_int64(4), 2, None, None, 5, d(0.1), d(1), d(1), d(5), 0, None) == -1
    assert b"out is null" in library.ds_last_error()
    cases = [(dict(feat=None), b"null"), (dict(n=0), b"rows"), (dict(nf=97), b"n_features"), (dict(depth=0), b"max_depth"),
             (dict(depth=9), b"max_depth"), (dict(eta=0.0), b"eta"), (dict(lam=0.0, mcw=0.0), b"eta"),
             (dict(offsets=np.array([1, 1, 2], np.int32)), b"cut_offsets[0]"),
             (dict(offsets=np.array([0, 2, 2], np.int32)), b"ascending"),
             (dict(offsets=np.array([0, 255, 255], np.int32), c=np.arange(255, dtype=np.float32)), b"cuts"),
             (dict(c=np.array([np.nan, 1], np.float32)), b"ascending")]
    for kwargs, message in cases:
        assert create(**kwargs) == -1, kwargs
        assert message in library.ds_last_error(), (kwargs, library.ds_last_error())
        assert not out.value
    labels = np.zeros(4, np.float32)
    assert library.ds_trainer_set_labels(None, labels.ctypes.data_as(p)) == -1
    assert b"null" in library.ds_last_error()
    assert library.ds_trainer_set_eval(None, None, None, ctypes.c_int64(1)) == -1
    assert library.ds_trainer_step(None, None, None, None) == -1
    assert b"null" in library.ds_last_error()
    assert library.ds_trainer_read(None, None, None, None, None, None) == -1
    assert b"null" in library.ds_last_error()
    library.ds_trainer_destroy(None)
