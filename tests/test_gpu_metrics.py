"""ds_auc_device / ds_auc / ds_weighted_logloss_device (csrc/ds_metrics.hip) against the NumPy oracle of the rule
(tests/metrics_oracle.py): all five AUC integers equal, the log-loss sum within one quantum per row.

The numbers of negatives sit at the edges of the shared radix sort (csrc/ds_radix.h): its wave (64), its scatter step
(kSortThreads = 256) and its tile (kSortTile = 8192), and a column of more than three tiles."""
import numpy as np
import pytest

import metrics_oracle as oracle

pytestmark = pytest.mark.gpu

NEGATIVES = (1, 63, 64, 65, 255, 256, 257, 8191, 8192, 8193, 3 * 8192 + 5)
POSITIVES = (1, 77, 1000)
DISTRIBUTIONS = ("bits", "unit", "four")


def make_scores(kind, n, rng):
    if kind == "bits":      # any bit pattern: both signs, denormals, and the special values placed where they fit
        scores = rng.randint(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32).copy()
        special = np.float32([np.inf, -np.inf, 0.0, -0.0, np.nan, -np.nan, np.inf, -0.0, 0.0, np.nan])
        at = rng.permutation(n)[:min(n, special.shape[0])]
        scores[at] = special[:at.shape[0]]
        return scores
    if kind == "unit":      # [1, 2): one exponent, so the two high digits are the same in every key
        return (1.0 + rng.rand(n)).astype(np.float32)
    if kind == "four":      # mass ties
        return rng.choice(np.float32([-2.5, 0.0, 1e-3, 7.0]), n).astype(np.float32)
    raise ValueError(kind)


def make_case(kind, n_neg, n_pos, seed):
    rng = np.random.RandomState(seed)
    labels = np.zeros(n_neg + n_pos, np.float32)
    labels[rng.permutation(n_neg + n_pos)[:n_pos]] = 1
    return make_scores(kind, n_neg + n_pos, rng), labels


def device_counts(scores, labels):
    import doppel_speller_amd as ds
    from doppel_speller_amd import _lib
    d_scores = _lib.DeviceArray.from_host(scores)
    try:
        return ds.auc_counts(d_scores, labels)
    finally:
        d_scores.free()


@pytest.mark.parametrize("kind", DISTRIBUTIONS)
@pytest.mark.parametrize("n_neg", NEGATIVES)
def test_auc_counts_equal_the_oracle(kind, n_neg):
    n_pos = POSITIVES[(NEGATIVES.index(n_neg) + DISTRIBUTIONS.index(kind)) % 3]
    scores, labels = make_case(kind, n_neg, n_pos, 100 + n_neg)
    expected = oracle.auc_counts(scores, labels)
    assert device_counts(scores, labels) == expected
    if kind != "bits":
        assert expected[2:] == (n_pos, n_neg, 0)


def test_every_positive_count_at_every_distribution():
    for kind in DISTRIBUTIONS:
        for n_pos in POSITIVES:
            scores, labels = make_case(kind, 257, n_pos, 7 * n_pos)
            assert device_counts(scores, labels) == oracle.auc_counts(scores, labels), (kind, n_pos)


def test_all_scores_equal_skips_every_pass():
    import doppel_speller_amd as ds
    labels = (np.arange(9000) % 3 == 0).astype(np.float32)
    scores = np.full(9000, 0.75, np.float32)
    assert device_counts(scores, labels) == oracle.auc_counts(scores, labels) == (0, 3000 * 6000, 3000, 6000, 0)
    assert ds.roc_auc(scores, labels) == 0.5


def test_an_empty_class():
    """No positives, then no negatives (no key to sort, no buffer to search): the class sizes are right, the pair counts
    are zero and the AUC is NaN."""
    import math
    import doppel_speller_amd as ds
    rng = np.random.RandomState(3)
    for n in (1, 300, 8193):
        scores = make_scores("bits", n, rng)
        nans = int(np.count_nonzero(np.isnan(scores)))
        for label in (0, 1):
            labels = np.full(n, label, np.float32)
            expected = oracle.auc_counts(scores, labels)
            assert expected == ((0, 0, 0, n - nans, nans) if label == 0 else (0, 0, n - nans, 0, nans))
            assert device_counts(scores, labels) == expected
            assert ds.auc_counts(scores, labels) == expected          # ds_auc, host arrays
            assert math.isnan(ds.roc_auc(scores, labels))


def test_result_does_not_depend_on_the_grid_and_repeats():
    from doppel_speller_amd import train
    scores, labels = make_case("bits", 3 * 8192 + 5, 1000, 11)
    expected = oracle.auc_counts(scores, labels)
    assert expected[4] > 0 and expected[0] > 0
    first = device_counts(scores, labels)
    assert first == expected and device_counts(scores, labels) == first      # two consecutive calls
    try:
        for cap in (1, 3):
            train.metrics_option("max_blocks", cap)
            assert device_counts(scores, labels) == expected, cap
    finally:
        train.metrics_option("max_blocks", 0)
    with pytest.raises(Exception, match="unknown option"):
        train.metrics_option("min_blocks", 1)


def test_host_and_device_forms_agree():
    import doppel_speller_amd as ds
    scores, labels = make_case("four", 8193, 77, 2)
    expected = oracle.auc_counts(scores, labels)
    assert ds.auc_counts(scores, labels) == expected
    from doppel_speller_amd import _lib
    d_scores = _lib.DeviceArray.from_host(scores)
    assert ds.roc_auc(d_scores, labels) == ds.roc_auc(scores, labels) == oracle.auc(expected)
    d_scores.free()
    with pytest.raises(ValueError, match="labels must all be 0 or 1"):
        ds.auc_counts(scores, labels + 2)


def test_weighted_logloss_against_the_oracle():
    """n = 10,000, margins in [-30, 30] and a few at +-5,000 that reach the cap.  A row's quantised term may differ from
    NumPy's by one unit of 2^-20 where the two libms differ in the last place of a float64, by nothing more: the sums
    are within n."""
    from doppel_speller_amd import train
    rng = np.random.RandomState(9)
    n = 10000
    margins = rng.uniform(-30, 30, n).astype(np.float32)
    margins[rng.permutation(n)[:6]] = np.float32([5000, -5000, 5000, -5000, 5000, -5000])
    labels = (rng.rand(n) < 0.3).astype(np.float32)
    labels[margins == 5000] = [0, 1, 0]
    labels[margins == -5000] = [1, 0, 1]
    expected_sum, expected_rows = oracle.logloss_counts(margins, labels, 5.0)
    capped = int(np.count_nonzero(oracle.logloss_terms(margins, labels, 5.0) == 2048 << 20))
    assert capped == 4                                       # 5,000 for a negative, -5,000 for a positive
    got = train.logloss_counts(margins, labels, 5.0)
    print("log loss: device", got[0], "oracle", expected_sum, "difference", got[0] - expected_sum)
    assert got[1] == expected_rows == n
    assert abs(got[0] - expected_sum) <= n
    assert train.logloss_counts(margins, labels, 5.0) == got                 # two runs
    assert train.logloss_counts(margins, labels, 1.0)[0] < got[0]
    assert abs(train.logloss_value((0, 0, 0, 0) + got) - oracle.logloss((expected_sum, n))) < 1e-6


def test_weighted_logloss_of_infinite_and_nan_margins():
    """No loss for an infinite margin on the row's own side, the cap on the other side and for a NaN: exact integers."""
    from doppel_speller_amd import train
    margins = np.float32([np.inf, -np.inf, np.inf, -np.inf, np.nan, np.nan])
    labels = np.float32([1, 0, 0, 1, 0, 1])
    assert oracle.logloss_counts(margins, labels, 5.0) == (4 * (2048 << 20), 6)
    assert train.logloss_counts(margins, labels, 5.0) == (4 * (2048 << 20), 6)
    assert train.logloss_counts(margins[:2], labels[:2], 5.0) == (0, 2)
