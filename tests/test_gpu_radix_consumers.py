"""radix_sort_columns (csrc/ds_radix.h) in every stage that stands on it, bit for bit against the NumPy oracles of those
stages: the isotonic fit (two columns of one sort), the AUC (one column, and the batch trainer's column per model), the
cuts (many columns of one launch).  The columns are those of tests/radix_cases.py: every one of the 16 patterns of
skipped passes, hence both buffers a column can end in, in columns of more than one sort tile, with padding longer than
a tile, beside columns of other patterns, and under active lists of the batch in which the position of a model is not
its number.  tests/test_radix_cases_cpu.py proves that the columns are what their names say."""
import numpy as np
import pytest

import calibration_oracle
import metrics_oracle
import radix_cases as cases
from cuts_cases import same_bits
from forest_train_oracle import make_data
from test_gpu_calibration import device_fit, host_fit, options, same
from test_gpu_cuts_device import check, device_cuts
from test_gpu_trainer_metrics import check_set

pytestmark = pytest.mark.gpu

FAMILIES = cases.calibration_families()


# ---- calibration: the negatives' and the positives' column of one fit -----------------------------------------------------
@pytest.fixture(scope="module")
def fits():
    """family -> name -> (scores, target, the oracle's fit), computed once."""
    out = {}
    for family, members in FAMILIES.items():
        out[family] = {}
        for name, mask_neg, mask_pos, n_neg, n_pos, nan_share in members:
            scores, target = cases.calibration_case(mask_neg, mask_pos, n_neg, n_pos, nan_share)
            out[family][name] = (scores, target, calibration_oracle.fit(scores, target))
    return out


def fit_in_every_form(scores, target, want, where):
    same(device_fit(scores, target), want, (where, "device"))
    same(host_fit(scores, target), want, (where, "host"))
    with options(segment_points=64, max_blocks=1):
        same(device_fit(scores, target), want, (where, "segment_points=64, max_blocks=1"))


@pytest.mark.parametrize("mask_neg", cases.MASKS, ids=lambda mask: f"{mask:04b}")
def test_small_fits_of_every_pair_of_skip_patterns(mask_neg, fits):
    """300 negatives and 211 positives: the 16 patterns of the positives beside this one of the negatives."""
    for name, a, b, _, _, _ in FAMILIES["small"]:
        if a != mask_neg:
            continue
        scores, target, want = fits["small"][name]
        assert want["n_nan"] == 0 and want["n_points"] >= 1
        fit_in_every_form(scores, target, want, name)


@pytest.mark.parametrize("family", ["large", "large_nan"])
@pytest.mark.parametrize("name", [member[0] for member in FAMILIES["large"]])
def test_fits_of_columns_longer_than_two_tiles_with_padding_longer_than_one(family, name, fits):
    """16,389 negatives and 8,193 positives in columns of 24,582 keys; then with 1 % NaN rows, which are dropped,
    counted and absent from the OR / AND."""
    scores, target, want = fits[family][name]
    assert (want["n_nan"] > 0) == (family == "large_nan")
    fit_in_every_form(scores, target, want, (family, name))


# ---- AUC: one column --------------------------------------------------------------------------------------------------------
def device_counts(scores, labels):
    import doppel_speller_amd as ds
    from doppel_speller_amd import _lib
    d_scores = _lib.DeviceArray.from_host(scores)
    try:
        return ds.auc_counts(d_scores, labels)
    finally:
        d_scores.free()


@pytest.mark.parametrize("n_neg", cases.AUC_NEGATIVES)
@pytest.mark.parametrize("name, mask, nan_negative", [case[:3] for case in cases.auc_family(0)],
                         ids=[case[0] for case in cases.auc_family(0)])
def test_auc_counts_at_every_skip_pattern(name, mask, nan_negative, n_neg):
    from doppel_speller_amd import train
    scores, labels = cases.auc_case(mask, n_neg, nan_negative)
    expected = metrics_oracle.auc_counts(scores, labels)
    assert expected[2:] == (cases.AUC_POSITIVES - 2, n_neg - int(nan_negative), 2 + int(nan_negative))
    assert expected[1] >= 331                                    # ties (one of the drawn values may be the NaN row)
    assert device_counts(scores, labels) == expected
    try:
        train.metrics_option("max_blocks", 1)
        assert device_counts(scores, labels) == expected, "max_blocks=1"
    finally:
        train.metrics_option("max_blocks", 0)


# ---- cuts: 80 columns of one matrix, in groups of changing company ------------------------------------------------------
@pytest.mark.parametrize("max_bin", [256, 16])
@pytest.mark.parametrize("n", cases.CUT_ROWS)
def test_cuts_of_columns_of_every_skip_pattern_in_one_launch(n, max_bin):
    from doppel_speller_amd.train import cuts_option
    x, columns = cases.cuts_matrix(n)
    names = [name for name, _, _ in columns]
    # the default group, all 80 columns in one launch: check() holds it against compute_cuts and the NumPy oracle
    want, want_offsets = check(x, max_bin, names)
    if max_bin == 256:                                          # every head of a `few` column is a cut
        for f, (name, _, distinct) in enumerate(columns):
            if distinct is not None:
                real = x[:, f][~np.isnan(x[:, f])]
                assert want_offsets[f + 1] - want_offsets[f] == np.unique(real).shape[0] - 1, name
    try:
        for group in (1, 5, x.shape[1]):
            cuts_option("column_group", group)
            cuts, offsets = device_cuts(x, max_bin)
            for f, name in enumerate(names):
                assert same_bits(cuts[offsets[f]:offsets[f + 1]], want[want_offsets[f]:want_offsets[f + 1]]), (name, group)
            assert offsets.tolist() == want_offsets.tolist(), group
    finally:
        cuts_option("column_group", 0)


# ---- the batch trainer's metrics: a column per active model --------------------------------------------------------------
ROWS = 14000
FOLD_ROWS = (12000, 1900, 65, 35)
SETS = [dict(max_depth=2), dict(max_depth=4, beta=2.0)]
MODELS = [dict(one, held_out=k) for one in SETS for k in range(4)]
ACTIVE = ([0, 1, 2, 3, 4, 5, 6, 7], [1, 4, 5], [7], [0, 2, 3, 6], [3])
BOTH = ("auc", "logloss")


@pytest.fixture(scope="module")
def batch_data():
    """Fold 0 holds more negatives than a sort tile, folds 2 and 3 are far smaller than the common key length, and fold
    3 holds positive rows only: a column without a key beside columns with keys."""
    x, y = make_data(ROWS, 12, 71)
    rng = np.random.RandomState(72)
    fold = np.zeros(ROWS, np.uint8)
    only_positives = rng.permutation(np.nonzero(y == 1)[0])[:FOLD_ROWS[3]]
    fold[only_positives] = 3
    rest = rng.permutation(np.setdiff1d(np.arange(ROWS), only_positives))
    fold[rest[:FOLD_ROWS[2]]] = 2
    fold[rest[FOLD_ROWS[2]:FOLD_ROWS[2] + FOLD_ROWS[1]]] = 1
    assert np.bincount(fold).tolist() == list(FOLD_ROWS)
    assert np.count_nonzero((fold == 0) & (y == 0)) > cases.TILE
    assert (y[fold == 3] == 1).all() and 0 < np.count_nonzero(y[fold == 2] == 0) < FOLD_ROWS[2]
    return x, y, fold


def skipped_parity(margins):
    """passes_done(OR ^ AND, 4) & 1 of a column's keys (no key: nothing differs from the cleared state, four passes)."""
    keys = metrics_oracle.keys(margins)
    differing = int(np.bitwise_or.reduce(keys) ^ np.bitwise_and.reduce(keys)) if keys.shape[0] else 0xFFFFFFFF
    return sum(1 for p in range(4) if (differing >> (8 * p)) & 0xFF) & 1


def run_batch(batch_data, metrics):
    """The rounds of ACTIVE -> (per round the table of the library and the heaps, the witnesses).  With metrics every
    active model is held against the oracle on its own margins, and every inactive model's row against the round
    before.  A witness is an active model whose position a in the list is not its number m while the column at a and
    the sort state under m (left there by this or an earlier round) end in different buffers."""
    import doppel_speller_amd as ds
    x, y, fold = batch_data
    batch = ds.ForestTrainerBatch().begin(x, y, fold, MODELS, metrics=metrics)
    record, witnesses, state = [], [], [None] * len(MODELS)
    try:
        before = None
        for round_, active in enumerate(ACTIVE):
            mask = np.zeros(len(MODELS), bool)
            mask[active] = True
            batch.step(mask)
            heaps = [None if h is None else (h[0].tobytes(), h[1].tobytes()) for h in batch.last_heap]
            if not metrics:
                record.append(dict(table=None, heaps=heaps))
                continue
            table = batch._metric_counts.copy()
            parities = []
            for m in active:
                held = fold == m % 4
                margins = batch.margins(m)[held]
                counts = batch.metric_counts[m][-1]
                assert counts == tuple(int(v) for v in table[m])
                check_set(counts, margins, y[held], MODELS[m].get("beta", 5.0), metrics, (m, round_))
                parities.append(skipped_parity(margins[y[held] == 0]))
            for m in range(len(MODELS)):
                if m not in active:
                    assert before is not None and np.array_equal(table[m], before[m]), (m, round_)
            for a, m in enumerate(active):
                state[a] = parities[a]
            for a, m in enumerate(active):
                negatives, positives = int(table[m][3]), int(table[m][2])
                if a != m and negatives and positives and state[m] != state[a]:
                    witnesses.append((round_, a, m))
            before = table
            record.append(dict(table=table, heaps=heaps))
        history = [list(curve) for curve in batch.history]
    finally:
        batch.close()
    return record, witnesses, history


def test_batch_metrics_under_active_lists_that_are_no_prefix(batch_data):
    """Eight models over four folds, five rounds: all models, [1, 4, 5], [7] (a fold without negatives, alone), [0, 2, 3,
    6] and [3].  The sort state is indexed by the position in the list and the counters by the model; the key length
    stays that of fold 0 whichever folds are active."""
    from doppel_speller_amd import tuning
    record, witnesses, history = run_batch(batch_data, BOTH)
    # the run can tell the two indices apart: somewhere the buffer parity under the position is not the one under the model
    assert witnesses, "no round in which the sort state at a and at m end in different buffers"
    last = record[-1]["table"]
    assert (last >= 0).all()
    for m in (3, 7):                                            # positives only: no pair, no negative
        assert last[m][:4].tolist() == [0, 0, FOLD_ROWS[3], 0] and last[m][5] == FOLD_ROWS[3]
    assert last[4][3] > cases.TILE                              # more than a tile of keys
    try:
        tuning.batch_option("max_blocks", 1)
        capped, _, capped_history = run_batch(batch_data, BOTH)
    finally:
        tuning.batch_option("max_blocks", 0)
    for a, b in zip(capped, record):
        assert np.array_equal(a["table"], b["table"]) and a["heaps"] == b["heaps"]
    plain, _, plain_history = run_batch(batch_data, ())
    assert [r["heaps"] for r in plain] == [r["heaps"] for r in record]
    assert plain_history == history == capped_history
