"""ForestTrainer on the GPU at the sizes and shapes where its launch geometry changes, against the NumPy oracle
(tests/forest_train_oracle.py) with the per-round checks of test_gpu_trainer.py: depth 8 with 96 features (two and
four node groups of histograms, a second split workgroup), odd feature counts, row sets past the row kernels' grid,
and max_bin below 256."""
import numpy as np
import pytest

import forest_train_oracle as oracle
from forest_train_oracle import make_data
from test_gpu_trainer import check_rounds

pytestmark = pytest.mark.gpu


def split_features(trees):
    return set(int(f) for tree in trees for f in tree["feature"][tree["state"] == oracle.SPLIT])


def test_depth_8_with_96_features_and_a_duplicate_last_feature():
    import doppel_speller_amd as ds
    x, y = oracle.deep_wide_data()
    ex, ey = oracle.deep_wide_data(20000, 8)
    p = oracle.DEEP
    trainer = ds.ForestTrainer().begin(x, y, ex, ey, **p)
    trees = check_rounds(trainer, x, y, ex, ey, 4, p["max_depth"], p["eta"], p["min_child_weight"], p["reg_lambda"])
    for round_, tree in enumerate(trees):
        second_group, second_workgroup, deepest_leaves = oracle.deep_paths(tree)
        assert second_group > 0 and second_workgroup > 0 and deepest_leaves > 0, (round_, oracle.deep_paths(tree))
    used = split_features(trees)
    assert 0 in used and 95 not in used, sorted(used)   # column 95 == column 0: every tie goes to the lower feature


def one_feature_wave(n, seed):
    """One feature, labels that flip along it: trees need every level to follow them."""
    x, _ = make_data(n, 1, seed)
    rng = np.random.RandomState(seed + 1)
    y = (np.sin(6 * x[:, 0]) + 0.5 * rng.randn(n) > 0).astype(np.float32)
    return x, y


@pytest.mark.parametrize("nf", [17, 1])
def test_depth_7_with_odd_feature_counts(nf):
    """nf = 17: 16 features per histogram group at level 0, the last group holds one feature.  nf = 1: one feature
    per group at every level, two node groups at level 6."""
    import doppel_speller_amd as ds
    if nf == 1:
        (x, y), (ex, ey) = one_feature_wave(30000, 8), one_feature_wave(10000, 18)
    else:
        (x, y), (ex, ey) = make_data(30000, nf, 24), make_data(10000, nf, 25)
    trainer = ds.ForestTrainer().begin(x, y, ex, ey, max_depth=7, eta=0.3, min_child_weight=0.5)
    trees = check_rounds(trainer, x, y, ex, ey, 4, 7, 0.3, 0.5, 1.0)
    for tree in trees:
        assert np.count_nonzero(tree["state"][95:127] == oracle.SPLIT) > 0     # level 6, second node group
        assert np.count_nonzero(tree["state"][127:255] == oracle.LEAF) > 0     # leaves at level 7
    assert nf - 1 in split_features(trees)                                    # the last feature group is used


def test_rows_past_the_row_kernels_grid():
    """row_grid launches at most 8 x compute units workgroups of 256 rows (8 x 256 x 256 = 524,288 rows per pass on
    the 256 CUs of an MI355X); more rows take further grid-stride passes in the gradient, partition and evaluation
    kernels.  The training margins go through ForestModel.predict at 1.2M rows, past the forest kernel's
    4096 x 256 = 1,048,576 rows per pass."""
    import doppel_speller_amd as ds
    n, n_eval = 1_200_000, 600_000
    assert n > 8 * 256 * 256 and n_eval > 8 * 256 * 256 and n > 4096 * 256
    x, y = make_data(n, 8, 31)
    ex, ey = make_data(n_eval, 8, 32)
    trainer = ds.ForestTrainer().begin(x, y, ex, ey, max_depth=5, eta=0.3)
    trees = check_rounds(trainer, x, y, ex, ey, 3, 5, 0.3, 1.0, 1.0)
    assert all(np.count_nonzero(tree["state"] == oracle.SPLIT) > 8 for tree in trees)


@pytest.mark.parametrize("max_bin", [16, 2])
def test_max_bin_below_256(max_bin):
    import doppel_speller_amd as ds
    x, y = make_data(20000, 12, 40 + max_bin)
    ex, ey = make_data(5000, 12, 41 + max_bin)
    trainer = ds.ForestTrainer().begin(x, y, ex, ey, max_depth=5, eta=0.3, max_bin=max_bin)
    per_feature = oracle.cuts(x, max_bin)
    assert np.array_equal(trainer.bins(), oracle.bins(x, per_feature))
    counts = [c.size for c in per_feature]
    trees = check_rounds(trainer, x, y, ex, ey, 4, 5, 0.3, 1.0, 1.0, max_bin=max_bin)
    if max_bin == 2:
        assert counts == [0] * 12                  # no feature has a cut: every tree is a single root leaf
        for tree in trees:
            assert tree["state"][0] == oracle.LEAF and np.count_nonzero(tree["state"]) == 1
    else:
        assert max(counts) == max_bin - 2          # quantile cuts at the limit
        assert all(np.count_nonzero(tree["state"] == oracle.SPLIT) > 1 for tree in trees)
