"""The restatements the GPU tests compare the kernels with, held against answers captured from the reference's OWN
train.py and predict.py bodies (tests/golden/make_golden_predict.py -> train_objective.npz, predict_stages.npz,
predict_end_to_end.npz, predict_two_chunks.npz): the
objective, `custom-error` and the error matrix, the close ratio with its pre-filter, the tie rules of the close and the
model step, the exact dict, the remaining pair list and the final table.  What stays restated underneath is the body of
Levenshtein.ratio (the generator's stand-in is the published rule) and xgboost's predict (planted probabilities).
"""
import numpy as np
import pytest

import forest_train_oracle as fto
import reference_stage_cases as rc
import sweep_cases
import title_cases

QUANTUM = 2.0 ** 30


# ---- train.py ----------------------------------------------------------------------------------------------------------

def test_gradients_against_the_float64_typed_capture():
    """forest_train_oracle.gradients against fast_weighted_log_loss on inputs widened to float64 (what numba computes):
    within one unit of 2^-30 on every row.  The two differ by a few float64 ulp at most (fastmath, the order of the
    operations), about 2^-50 at |g| <= 5, so only a value on a rounding boundary can move, and by one unit.
    Rows that differ at all, counted here on the CPU: 0 of 4,000."""
    g = rc.OBJECTIVE
    assert int(g["beta"]) == 5 and g["p"].dtype == np.float32 and g["p"].shape[0] == 4000
    got = fto.gradients(g["p"], g["y"], 5.0)
    want = np.stack([np.rint(g["g64"] * QUANTUM), np.rint(g["h64"] * QUANTUM)], axis=1).astype(np.int64)
    differ = int((got != want).any(axis=1).sum())
    print(f"rows whose quantised gradient or hessian differs from the float64 capture: {differ} of {got.shape[0]}")
    assert np.abs(got - want).max() <= 1
    assert differ == 0                                  # the documented count; one-unit moves would show here first
    # the edges are in: 0, 1, the smallest denormal, both float32 neighbours of 0.5, 0.9 and 1.0, with both labels
    edges = [np.float32(0), np.float32(1e-45)]
    for value in (0.5, 0.9, 1.0):
        edges += [np.nextafter(np.float32(value), np.float32(0)), np.float32(value), np.nextafter(np.float32(value), np.float32(2))]
    for edge in edges:
        assert ((g["p"] == edge) & (g["y"] == 0)).any() and ((g["p"] == edge) & (g["y"] == 1)).any(), edge


def test_gradients_against_the_float32_typed_capture():
    """The same against the reference's source as NumPy evaluates it on float32 inputs: three float32 roundings at a
    magnitude of 5 at most, 2^-20.  `typing_differs` marks the rows where the two captures part after quantisation."""
    g = rc.OBJECTIVE
    got = fto.gradients(g["p"], g["y"], 5.0).astype(np.float64) / QUANTUM
    assert np.abs(got[:, 0] - g["g32"].astype(np.float64)).max() <= 2.0 ** -20
    assert np.abs(got[:, 1] - g["h32"].astype(np.float64)).max() <= 2.0 ** -20
    parts = (np.rint(g["g64"] * QUANTUM) != np.rint(g["g32"].astype(np.float64) * QUANTUM)) | \
        (np.rint(g["h64"] * QUANTUM) != np.rint(g["h32"].astype(np.float64) * QUANTUM))
    assert np.array_equal(parts, g["typing_differs"]) and parts.any() and not parts.all()


def test_custom_error_is_the_float64_typed_capture_at_every_threshold():
    """forest_train_oracle.custom_error restates fast_custom_error as numba types it: a float64 compare.  At 0.6, whose
    float32 lies above it, the float32 nearest to the threshold is positive there and negative as NumPy compares."""
    g = rc.OBJECTIVE
    p, y = g["planted_p"], g["planted_y"]
    for i, threshold in enumerate(g["thresholds"].tolist()):
        assert fto.custom_error(p, y, threshold) == int(g["custom_error_f64"][i]), threshold
        positive = np.array([fto.custom_error(p[r:r + 1], y[r:r + 1], threshold) == (0 if y[r] else 5)
                             for r in range(p.shape[0])])
        assert np.array_equal(positive, g["positive_f64"][i]), threshold
        nearest = p == np.float32(threshold)
        assert nearest.sum() == 2 and (p == np.nextafter(np.float32(threshold), np.float32(0))).sum() == 2
        assert np.array_equal(g["typings_disagree"][i], nearest & (np.float64(np.float32(threshold)) > threshold))
    assert g["typings_disagree"].sum(axis=1).tolist() == [0, 0, 2, 0]       # 0.9, 0.5, 0.6, 0.7
    assert int(g["custom_error_f64"][2]) != int(g["custom_error_f32"][2])


class _Planted:
    def __init__(self, planted):
        self.planted = planted

    def predict(self, features):
        assert features.shape[0] == self.planted.shape[0]
        return self.planted.copy()


@pytest.mark.parametrize("as_type", [float, np.float64, np.float32])
def test_error_matrix_is_the_capture_at_every_threshold(as_type):
    """train._error_matrix and train.evaluation_error_matrix restate get_evaluation_error_matrix, which compares the
    float32 predictions with the threshold as NumPy does, in float32, however the threshold is typed."""
    from doppel_speller_amd import train
    g = rc.OBJECTIVE
    p, y = g["planted_p"], g["planted_y"]
    for i, threshold in enumerate(g["thresholds"].tolist()):
        want = tuple(int(v) for v in g["error_matrix"][i])
        assert train._error_matrix(p, y, as_type(threshold)) == want, threshold
        features = np.zeros((p.shape[0], 3), dtype=np.float32)
        assert train.evaluation_error_matrix(_Planted(p), features, y, as_type(threshold)) == want, threshold
        tp, tn, fp, fn = want
        assert fn + 5 * fp == int(g["custom_error_f32"][i])
        assert np.array_equal(g["positive_matrix"][i], g["positive_f32"][i])


# ---- predict.py: the close ratio -----------------------------------------------------------------------------------------

def _encoded_pairs():
    import doppel_speller_amd as ds
    x_enc, x_len = ds.encode_titles(rc.PAIR_X)
    y_enc, y_len = ds.encode_titles(rc.PAIR_Y)
    return x_enc, x_len, y_enc, y_len


def test_close_ratios_and_the_zeroing_pre_filter(oracle):
    import doppel_speller_amd as ds
    g = rc.STAGES
    x_enc, x_len, y_enc, y_len = _encoded_pairs()
    assert [len(t) for t in rc.PAIR_X] == x_len.tolist() and [len(t) for t in rc.PAIR_Y] == y_len.tolist()
    got = oracle.close_ratios(x_len, y_len, x_enc, y_enc, ds.SPACE_CODE, ds.SORT_KEY, rc.LEVENSHTEIN_THRESHOLD)
    assert np.array_equal(got.astype(np.int64), g["pair_ratio"])
    zeroed = g["pair_deletion_ratio"] < rc.LEVENSHTEIN_THRESHOLD
    assert (got[zeroed] == 0).all() and zeroed.sum() >= 10 and (g["pair_deletion_ratio"] == 94).any()
    assert (g["pair_plain_ratio"][zeroed] > 0).any()                 # the pre-filter zeroes, the ratio alone would not
    # the three parts the sweep reads a ratio from: the pre-filter's floor, the plain and the token-sort ratio
    d, r, s = sweep_cases.close_parts(oracle, x_len, y_len, x_enc, y_enc, ds.SPACE_CODE, ds.SORT_KEY)
    assert np.array_equal(d.astype(np.int64), np.floor(g["pair_deletion_ratio"]).astype(np.int64))
    assert np.array_equal(r.astype(np.int64), g["pair_plain_ratio"])
    assert np.array_equal(s.astype(np.int64), g["pair_token_sort_ratio"])
    assert np.array_equal(sweep_cases.value_at(d, r, s, rc.LEVENSHTEIN_THRESHOLD).astype(np.int64), g["pair_ratio"])
    # what the pairs were made for
    plain, lifted = g["pair_plain_ratio"], g["pair_ratio"]
    assert (plain == 94).sum() >= 4 and (plain == 95).sum() >= 4 and ((plain <= 94) & (lifted > 94)).sum() >= 8
    assert {1, 3, 255} <= set(x_len.tolist()) | set(y_len.tolist())


def _rows_of(ids):
    row_of = {int(title_id): row for row, title_id in enumerate(rc.TRUTH_IDS)}
    return np.array([row_of.get(int(i), -1) for i in ids], dtype=np.int64)


def test_best_from_ratios_is_the_close_step(oracle):
    """The captured ratios of every candidate through title_cases.best_from_ratios against what _find_close_matches
    saved: a tie at the maximum and a maximum of exactly 94 leave the title to the model."""
    exact, close, _ = rc.stage_ids(0)
    best = title_cases.best_from_ratios(rc.RATIOS, rc.ROWS, rc.LEVENSHTEIN_THRESHOLD)
    reached = exact == rc.NOT_FOUND                                   # the titles the close step saw
    assert np.array_equal(rc.ids_of(best)[reached], close[reached])
    top = rc.RATIOS.max(axis=1)
    tied = (rc.RATIOS == top[:, None]).sum(axis=1) > 1
    assert (reached & tied & (top > 94) & (close == rc.NOT_FOUND)).sum() >= 4        # ties: no close match
    assert (reached & (top == 94) & (close == rc.NOT_FOUND)).sum() >= 2              # exactly 94: none
    assert (reached & (top == 95) & (close != rc.NOT_FOUND)).sum() >= 1
    # and the oracle's ratios of those candidates are the captured ones
    import doppel_speller_amd as ds
    q_enc, q_len = ds.encode_titles(rc.TITLES)
    t_enc, t_len = ds.encode_titles(rc.TRUTH_TITLES)
    pair_q, pair_t = np.repeat(np.arange(rc.N_TITLES), rc.TOP_N), rc.ROWS.reshape(-1)
    got = oracle.close_ratios(q_len[pair_q], t_len[pair_t], q_enc[pair_q], t_enc[pair_t], ds.SPACE_CODE, ds.SORT_KEY,
                              rc.LEVENSHTEIN_THRESHOLD)
    assert np.array_equal(got.reshape(rc.ROWS.shape).astype(np.int64), rc.RATIOS)


# ---- predict.py: the pair list, the model step, the final table ---------------------------------------------------------

def test_remaining_pairs_and_select_matches(oracle):
    g = rc.STAGES
    exact, close, _ = rc.stage_ids(0)
    best = _rows_of(np.where(exact != rc.NOT_FOUND, exact, close))
    pair_q, pair_t = oracle.remaining_pairs(best, rc.ROWS)
    assert np.array_equal(pair_q, g["remaining_q"]) and np.array_equal(rc.ids_of(pair_t), g["remaining_id"])
    assert np.array_equal(rc.RATIOS[pair_q, np.arange(pair_q.shape[0]) % rc.TOP_N], g["remaining_ratio"])
    planted = rc.remaining_probabilities(pair_q)
    for i, threshold in enumerate(rc.THRESHOLDS):
        _, _, model = rc.stage_ids(i)
        match_q, match_t = oracle.select_matches(pair_q, pair_t, planted, rc.TOP_N, threshold)
        got = np.full(rc.N_TITLES, rc.NOT_FOUND, dtype=np.int64)
        got[match_q] = rc.ids_of(match_t)
        assert np.array_equal(got, model), threshold
    # what the cases were made for, at the reference's own threshold
    _, _, model = rc.stage_ids(0)
    top = rc.PROBABILITIES.max(axis=1)
    reached = np.zeros(rc.N_TITLES, dtype=bool)
    reached[pair_q] = True
    nearest = np.float32(0.9)
    assert (reached & (top == nearest) & (model == rc.NOT_FOUND)).sum() == 1
    assert (reached & (top == np.nextafter(nearest, np.float32(1))) & (model != rc.NOT_FOUND)).sum() == 1
    tied = (rc.PROBABILITIES == top[:, None]).sum(axis=1) > 1
    assert (reached & tied & (top > nearest) & (model == rc.NOT_FOUND)).sum() >= 4


def test_the_four_stage_restatement_and_the_final_table(oracle):
    """tests/prediction_restatement.py, the judge of tests/test_gpu_prediction.py, on the captured titles and planted
    candidates, and the host drivers behind Prediction (combine_stages, finalize_output, predictions_accuracy)."""
    from doppel_speller_amd import prediction
    from prediction_restatement import Expected
    g = rc.STAGES
    expected = Expected(rc.TRUTH_TITLES, rc.TITLES, rc.TOP_N, oracle, rows=rc.ROWS,
                        levenshtein_threshold=rc.LEVENSHTEIN_THRESHOLD)
    exact, close, _ = rc.stage_ids(0)
    assert np.array_equal(rc.ids_of(expected.exact), exact)
    assert np.array_equal(rc.ids_of(np.where(expected.exact >= 0, -1, expected.close)), close)
    assert np.array_equal(expected.ratios.astype(np.int64), rc.RATIOS)
    assert np.array_equal(expected.pair_q, g["remaining_q"]) and np.array_equal(rc.ids_of(expected.pair_t), g["remaining_id"])
    names = np.array(rc.NAMES)
    for copies in (2, 3):                                              # the last of the rows that hold the title wins
        for q in np.nonzero(names == f"exact_{copies}")[0]:
            held = [row for row, title in enumerate(rc.TRUTH_TITLES) if title == rc.TITLES[q]]
            assert len(held) == copies and exact[q] == rc.TRUTH_IDS[held[-1]] != rc.TRUTH_IDS[held[0]]
    planted = rc.remaining_probabilities(expected.pair_q)
    for i, threshold in enumerate(rc.THRESHOLDS):
        _, _, model = rc.stage_ids(i)
        model_rows = expected.model_rows(planted, threshold, oracle)
        assert np.array_equal(rc.ids_of(model_rows), model), threshold
        final = expected.final_rows(model_rows)
        assert np.array_equal(rc.ids_of(final), rc.final_ids(i)), threshold
        row, stage = prediction.combine_stages(expected.exact, np.where(expected.exact >= 0, -1, expected.close), model_rows)
        assert np.array_equal(row, final)
        assert np.array_equal(stage == prediction.STAGE_MODEL, model != rc.NOT_FOUND)
        frame = prediction.finalize_output(np.arange(rc.N_TITLES)[::-1], final[::-1], rc.TRUTH_IDS)
        assert list(frame.columns) == ["title_id", "test_index"]
        assert np.array_equal(frame["title_id"].to_numpy(), g[f"final_id_{i}"])
        assert np.array_equal(frame["test_index"].to_numpy(), g[f"final_index_{i}"])
        counts = prediction.predictions_accuracy(rc.final_ids(i), g["actual_ids"])
        assert [counts[key] for key in prediction.ACCURACY_KEYS] == g[f"counts_{i}"].tolist(), threshold
    assert (rc.final_ids(0) == rc.NOT_FOUND).sum() >= 10 and len({tuple(rc.final_ids(i)) for i in range(4)}) == 4


def test_the_restatement_behind_the_reference_match_maker(oracle):
    """predict_end_to_end.npz: the candidates are those of the reference's own MatchMaker (top_n = 4), the probabilities
    planted for exactly those.  The restatement with its own Jaccard stage finds the same candidates and the same table."""
    from prediction_restatement import Expected
    e = rc.END_TO_END
    k = int(e["top_n"])
    expected = Expected(rc.E2E_TRUTH_TITLES, rc.E2E_TITLES, k, oracle)
    got = rc.E2E_TRUTH_IDS[expected.rows]
    assert np.array_equal(np.sort(got, axis=1), np.sort(e["candidate_ids"], axis=1)) and e["jaccard_gap"].min() > 0.1
    ids = lambda rows: np.where(np.asarray(rows) >= 0, rc.E2E_TRUTH_IDS[np.maximum(rows, 0)], rc.NOT_FOUND)
    exact, close, model = rc.e2e_stage_ids()
    assert np.array_equal(ids(expected.exact), exact)
    assert np.array_equal(ids(np.where(expected.exact >= 0, -1, expected.close)), close)
    margin = {(q, int(i)): m for q in range(len(rc.E2E_TITLES)) for i, m in zip(e["candidate_ids"][q], e["margins"][q])}
    margins = np.array([margin[(int(q), int(rc.E2E_TRUTH_IDS[t]))] for q, t in zip(expected.pair_q, expected.pair_t)],
                       dtype=np.float32)
    planted = np.float32(1) / (np.float32(1) + np.exp(-margins, dtype=np.float32))
    model_rows = expected.model_rows(planted, float(e["threshold"]), oracle)
    assert np.array_equal(ids(model_rows), model)
    assert np.array_equal(ids(expected.final_rows(model_rows)), e["final_id"])
    assert np.array_equal(e["final_index"], np.arange(len(rc.E2E_TITLES)))
    # the lookup tree of the GPU test gives every captured pair its planted margin and any other pair the default
    row_of = {int(title_id): row for row, title_id in enumerate(rc.E2E_TRUTH_IDS)}
    truth_lengths = np.array([[len(rc.E2E_TRUTH_TITLES[row_of[int(i)]]) for i in row] for row in e["candidate_ids"]])
    title_lengths = [len(t) for t in rc.E2E_TITLES]
    forest = rc.pair_lookup_forest(title_lengths, truth_lengths, e["margins"], float(e["default_margin"]))

    def walk(a, b):
        at = 0
        while forest["feature"][at] >= 0:
            value = (a, b)[forest["feature"][at]]
            at = forest["yes"][at] if value < forest["threshold"][at] else forest["no"][at]
        return forest["threshold"][at]

    for q in range(len(rc.E2E_TITLES)):
        for slot in range(k):
            assert walk(title_lengths[q], truth_lengths[q, slot]) == e["margins"][q, slot]
        assert walk(title_lengths[q], 300) == e["default_margin"] and walk(300, truth_lengths[q, 0]) == e["default_margin"]


def test_the_two_chunk_run_of_generate_test_predictions(oracle):
    """predict_two_chunks.npz: the reference's generate_test_predictions itself on the 10,003 titles of
    tests/chunk_cases.py (top_n = 2), which its loop cuts into chunks of 10,000 and 3.  The restatement, which knows no
    chunks, gives the same table; the three titles of the second chunk repeat titles 1, 2, 3 and get their answers."""
    import chunk_cases as cc
    from doppel_speller_amd import prediction
    from prediction_restatement import Expected
    final_id = rc._load("predict_two_chunks.npz")["final_id"]
    truth_ids, rows, planted = cc.truth_ids(), cc.rows(), cc.probabilities()
    expected = Expected(cc.truth_titles(), cc.titles(), cc.TOP_N, oracle, rows=rows)
    model_rows = expected.model_rows(planted[expected.pair_q, np.arange(expected.pair_q.shape[0]) % cc.TOP_N], 0.9, oracle)
    final = expected.final_rows(model_rows)
    frame = prediction.finalize_output(np.arange(cc.N_TITLES), final, truth_ids)
    assert np.array_equal(frame["title_id"].to_numpy(), final_id)
    assert np.array_equal(final_id[cc.CHUNK:], final_id[1:4]) and final_id.shape[0] == cc.N_TITLES
    _, stage = prediction.combine_stages(expected.exact, np.where(expected.exact >= 0, -1, expected.close), model_rows)
    assert np.bincount(stage, minlength=4).min() >= 1000                 # every stage decides a thousand titles and more
    assert (final_id[::5][3::40] == truth_ids[31]).all()                 # the last of the three rows of that title
