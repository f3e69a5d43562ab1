"""The device entry points of the prediction stages on inputs captured from the reference, compared DIRECTLY with the
answers the reference's own predict.py and train.py bodies gave (tests/golden/make_golden_predict.py ->
predict_stages.npz, train_objective.npz; loaded by tests/reference_stage_cases.py), not with the oracle: the close ratio and
its cut, the tie rules of the close and the model step, the last-row-wins exact table, the remaining pair list, the ranked
slots, the sweep's counters and the outcome codes.

The device gradient cannot be given planted probabilities (the trainer computes them from its own margins).  It stays
pinned through the chain device == forest_train_oracle.gradients (tests/test_gpu_trainer*.py) == the reference
(tests/test_reference_stages_cpu.py).  The outcome codes take margins, not probabilities: the test below walks margins
across each threshold, holds the code against the captured verdict wherever the device's own probability IS a planted
float32 (the nearest to the threshold and its upper neighbour at every threshold, the lower one too at 0.6 and 0.7), and
against the captured verdicts of the threshold's neighbours everywhere else.

Prediction.generate_test_predictions and Prediction.ranked_matches run end to end on predict_end_to_end.npz: titles whose
candidates the reference's own MatchMaker chose (top_n = 4, no near-tie at the cut), with a probability planted for exactly
those; the model here is one lookup tree over construct_features' two length columns that gives every pair its planted
margin, so ties, order and the side of 0.9 are the planted ones.
"""
import ctypes

import numpy as np
import pytest

import reference_stage_cases as rc

pytestmark = pytest.mark.gpu
NULL = ctypes.c_void_p(0)


def _table(titles):
    import doppel_speller_amd as ds
    enc, lengths = ds.encode_titles(titles)
    return ds.TitleTable(enc, lengths)


def _sync():
    from doppel_speller_amd import _lib
    _lib.check(_lib.lib().ds_stream_sync(None, 0), "sync")


def _close_matches(queries, truth, rows, threshold):
    """ds_close_matches_device -> (ratios int64[Q, k], best_row int32[Q])."""
    import doppel_speller_amd as ds
    from doppel_speller_amd import _lib
    n, k = rows.shape
    d_rows, d_key = _lib.DeviceArray.from_host(rows.astype(np.int32)), _lib.DeviceArray.from_host(ds.SORT_KEY)
    d_ratios, d_best = _lib.DeviceArray((n, k), np.uint8), _lib.DeviceArray((n,), np.int32)
    _lib.check(_lib.lib().ds_close_matches_device(queries.handle, truth.handle, d_rows.ptr, 0, k, n, ds.SPACE_CODE,
                                                  d_key.ptr, threshold, d_ratios.ptr, d_best.ptr, NULL), "close")
    _sync()
    return d_ratios.to_host().astype(np.int64), d_best.to_host()


def _rows_of(ids):
    row_of = {int(title_id): row for row, title_id in enumerate(rc.TRUTH_IDS)}
    return np.array([row_of.get(int(i), -1) for i in ids], dtype=np.int32)


@pytest.fixture(scope="module")
def tables():
    return _table(rc.TITLES), _table(rc.TRUTH_TITLES)


def test_close_ratios_of_the_captured_title_pairs():
    """Every captured pair as a query with one candidate: the ratio of _get_levenshtein_ratio, zeroed by the pre-filter,
    lifted by the token-sort ratio, and the best row exactly where it is above 94."""
    g = rc.STAGES
    n = len(rc.PAIR_X)
    rows = np.arange(n, dtype=np.int32)[:, None]
    ratios, best = _close_matches(_table(rc.PAIR_X), _table(rc.PAIR_Y), rows, rc.LEVENSHTEIN_THRESHOLD)
    bad = np.nonzero(ratios[:, 0] != g["pair_ratio"])[0]
    assert bad.shape[0] == 0, [(rc.PAIR_X[i], rc.PAIR_Y[i], int(ratios[i, 0]), int(g["pair_ratio"][i])) for i in bad[:5]]
    assert np.array_equal(best, np.where(g["pair_ratio"] > rc.LEVENSHTEIN_THRESHOLD, rows[:, 0], -1))
    assert (g["pair_ratio"] == 94).sum() >= 4 and (g["pair_ratio"] == 95).sum() >= 4      # both sides of the cut


def test_close_parts_of_the_captured_title_pairs():
    """ds_close_parts_device with nothing skipped: the floor of the pre-filter's value, the plain and the token-sort
    ratio of the reference."""
    import doppel_speller_amd as ds
    from doppel_speller_amd import _lib
    g = rc.STAGES
    n = len(rc.PAIR_X)
    queries, truth = _table(rc.PAIR_X), _table(rc.PAIR_Y)
    d_rows = _lib.DeviceArray.from_host(np.arange(n, dtype=np.int32))
    d_key = _lib.DeviceArray.from_host(ds.SORT_KEY)
    parts = [_lib.DeviceArray((n,), np.uint8) for _ in range(3)]
    _lib.check(_lib.lib().ds_close_parts_device(queries.handle, truth.handle, d_rows.ptr, 0, 1, n, ds.SPACE_CODE, d_key.ptr,
                                                0, 100, parts[0].ptr, parts[1].ptr, parts[2].ptr, NULL), "parts")
    _sync()
    d, r, s = (part.to_host().astype(np.int64) for part in parts)
    assert np.array_equal(d, np.floor(g["pair_deletion_ratio"]).astype(np.int64))
    assert np.array_equal(r, g["pair_plain_ratio"])
    assert np.array_equal(s, g["pair_token_sort_ratio"])


def test_close_step_on_the_captured_candidates(tables):
    """The ratios of every planted candidate and the close step's single answer: none for two candidates tied at the
    maximum, none for a maximum of exactly 94."""
    queries, truth = tables
    ratios, best = _close_matches(queries, truth, rc.ROWS, rc.LEVENSHTEIN_THRESHOLD)
    assert np.array_equal(ratios, rc.RATIOS)
    exact, close, _ = rc.stage_ids(0)
    reached = exact == rc.NOT_FOUND                       # the reference's close step never sees an exact match
    assert np.array_equal(rc.ids_of(best)[reached], close[reached])
    names = np.array(rc.NAMES)
    for name in ("close_tie_then_model", "close_tie_then_none", "close_tie_then_model_tie", "close_token_sort_tie",
                 "twice_close_tie", "close_94_then_model", "close_94_then_none"):
        q = int(np.nonzero(names == name)[0][0])
        assert best[q] == -1 and rc.RATIOS[q].max() >= 94, name
        assert (rc.RATIOS[q] == rc.RATIOS[q].max()).sum() >= (1 if "94" in name else 2), name
    q = int(np.nonzero(names == "close_94_and_95")[0][0])
    assert sorted(rc.RATIOS[q].tolist())[-2:] == [94, 95] and rc.ids_of(best[q:q + 1])[0] == close[q] != rc.NOT_FOUND


def test_exact_matches_on_the_captured_titles(tables):
    """ds_exact_matches_device: the id the reference's reversed dict holds, the LAST row of a title held two or three times;
    and the override of the close step's best row."""
    from doppel_speller_amd import _lib
    queries, truth = tables
    exact, close, _ = rc.stage_ids(0)
    n = rc.N_TITLES
    before = _rows_of(close)
    d_exact, d_best = _lib.DeviceArray((n,), np.int32), _lib.DeviceArray.from_host(before)
    _lib.check(_lib.lib().ds_exact_matches_device(truth.handle, queries.handle, 0, n, d_exact.ptr, d_best.ptr, NULL),
               "exact")
    _sync()
    rows = d_exact.to_host()
    assert np.array_equal(rc.ids_of(rows), exact)
    assert np.array_equal(d_best.to_host(), np.where(rows >= 0, rows, before))
    names = np.array(rc.NAMES)
    for copies in (2, 3):
        for q in np.nonzero(names == f"exact_{copies}")[0]:
            held = [row for row, title in enumerate(rc.TRUTH_TITLES) if title == rc.TITLES[q]]
            assert len(held) == copies and rows[q] == held[-1]


def test_remaining_pairs_and_select_matches_on_the_planted_probabilities():
    """The pair list of the titles neither earlier stage matched, in the reference's order, and the model step at every
    captured threshold: a maximum equal to the float32 nearest to the threshold is no match, its upper neighbour is one,
    two candidates tied at the maximum are none."""
    from doppel_speller_amd import _lib
    lib = _lib.lib()
    g = rc.STAGES
    exact, close, _ = rc.stage_ids(0)
    n, k = rc.N_TITLES, rc.TOP_N
    best = _rows_of(np.where(exact != rc.NOT_FOUND, exact, close))
    d_best, d_rows = _lib.DeviceArray.from_host(best), _lib.DeviceArray.from_host(rc.ROWS)
    d_pair_q, d_pair_t = _lib.DeviceArray((n * k,), np.int32), _lib.DeviceArray((n * k,), np.int32)
    d_counts = _lib.DeviceArray((int(lib.ds_remaining_pairs_counts_size(n)),), np.int64)
    _lib.check(lib.ds_remaining_pairs_device(d_best.ptr, d_rows.ptr, n, k, 0, d_pair_q.ptr, d_pair_t.ptr, d_counts.ptr,
                                             NULL), "pairs")
    _sync()
    n_remaining, n_pairs = (int(v) for v in d_counts.to_host()[:2])
    assert n_pairs == n_remaining * k == g["remaining_q"].shape[0]
    pair_q, pair_t = d_pair_q.to_host()[:n_pairs], d_pair_t.to_host()[:n_pairs]
    assert np.array_equal(pair_q, g["remaining_q"]) and np.array_equal(rc.ids_of(pair_t), g["remaining_id"])
    d_planted = _lib.DeviceArray.from_host(rc.remaining_probabilities(pair_q))
    d_match_q, d_match_t = _lib.DeviceArray((n_remaining,), np.int32), _lib.DeviceArray((n_remaining,), np.int32)
    names = np.array(rc.NAMES)
    for i, threshold in enumerate(rc.THRESHOLDS):
        _lib.check(lib.ds_select_matches_device(d_pair_q.ptr, d_pair_t.ptr, d_planted.ptr, n_remaining, k, threshold,
                                                d_match_q.ptr, d_match_t.ptr, NULL), "select")
        _sync()
        got = np.full(n, rc.NOT_FOUND, dtype=np.int64)
        got[d_match_q.to_host()] = rc.ids_of(d_match_t.to_host())
        model = rc.stage_ids(i)[2]
        assert np.array_equal(got, model), threshold
        at, above = (int(np.nonzero(names == f"model_{where}_{threshold}")[0][0]) for where in ("at", "up"))
        assert got[at] == rc.NOT_FOUND and got[above] != rc.NOT_FOUND, threshold
        for name in ("model_tie_2", "model_tie_3", "model_tie_at_one", "twice_tied_maximum", "close_tie_then_model_tie"):
            assert got[int(np.nonzero(names == name)[0][0])] == rc.NOT_FOUND, name


def test_rank_matches_slot_0_is_the_reference_answer():
    """ds_rank_matches_device on the planted rows, probabilities and ratios with the captured exact and close rows: slot
    0 is the reference's single answer wherever the reference gives one, at every captured threshold."""
    from doppel_speller_amd import _lib
    exact, close, _ = rc.stage_ids(0)
    n, k, slots = rc.N_TITLES, rc.TOP_N, 2
    d_in = [_lib.DeviceArray.from_host(a) for a in (rc.ROWS, rc.PROBABILITIES, rc.RATIOS.astype(np.uint8),
                                                    _rows_of(exact), _rows_of(close))]
    out = (_lib.DeviceArray((n, slots), np.int32), _lib.DeviceArray((n, slots), np.float32),
           _lib.DeviceArray((n, slots), np.uint8), _lib.DeviceArray((n, slots), np.int8))
    _lib.check(_lib.lib().ds_rank_matches_device(*(a.ptr for a in d_in), n, k, slots, rc.N_TRUTH, *(a.ptr for a in out),
                                                 NULL), "rank")
    _sync()
    rows, stages = out[0].to_host(), out[3].to_host()
    head = rc.ids_of(rows[:, 0])
    answered = 0
    for i in range(len(rc.THRESHOLDS)):
        final = rc.final_ids(i)
        given = final != rc.NOT_FOUND
        assert np.array_equal(head[given], final[given]), rc.THRESHOLDS[i]
        answered += int(given.sum())
    assert answered > 100
    assert np.array_equal(stages[:, 0] == 1, exact != rc.NOT_FOUND)
    assert np.array_equal(stages[:, 0] == 2, close != rc.NOT_FOUND)


def test_threshold_sweep_cells_are_the_captured_counts(tables):
    """ds_close_parts_device and ds_threshold_sweep_device on the captured titles, planted candidates and probabilities:
    the cell at (94, every captured probability threshold) holds the four counters the reference's own counting loop
    (cli.py:107-120) printed for its final table."""
    import doppel_speller_amd as ds
    from doppel_speller_amd import _lib
    lib = _lib.lib()
    queries, truth = tables
    g = rc.STAGES
    n, k = rc.N_TITLES, rc.TOP_N
    exact = _rows_of(rc.stage_ids(0)[0])
    order = np.argsort(rc.THRESHOLDS)
    lev = np.array([rc.LEVENSHTEIN_THRESHOLD], dtype=np.int32)
    prob = np.array(rc.THRESHOLDS, dtype=np.float32)[order]
    d_rows, d_key = _lib.DeviceArray.from_host(rc.ROWS), _lib.DeviceArray.from_host(ds.SORT_KEY)
    parts = [_lib.DeviceArray((n, k), np.uint8) for _ in range(3)]
    _lib.check(lib.ds_close_parts_device(queries.handle, truth.handle, d_rows.ptr, 0, k, n, ds.SPACE_CODE, d_key.ptr,
                                         int(lev[0]), int(lev[0]), parts[0].ptr, parts[1].ptr, parts[2].ptr, NULL), "parts")
    d_in = [_lib.DeviceArray.from_host(a) for a in (rc.PROBABILITIES, exact, rc.actual_rows(), lev, prob)]
    d_counts = _lib.DeviceArray.from_host(np.zeros(prob.shape[0] * 4, dtype=np.int64))
    _lib.check(lib.ds_threshold_sweep_device(d_rows.ptr, parts[0].ptr, parts[1].ptr, parts[2].ptr, d_in[0].ptr, d_in[1].ptr,
                                             d_in[2].ptr, n, k, d_in[3].ptr, 1, d_in[4].ptr, prob.shape[0], d_counts.ptr,
                                             NULL), "sweep")
    _sync()
    counts = d_counts.to_host().reshape(prob.shape[0], 4)
    for cell, i in enumerate(order):
        assert counts[cell].tolist() == g[f"counts_{i}"][:4].tolist(), rc.THRESHOLDS[i]
        assert int(counts[cell, 3] + 5 * counts[cell, 1]) == int(g[f"counts_{i}"][4])
    assert len({tuple(c) for c in counts.tolist()}) == prob.shape[0]          # every threshold moves a title


def test_outcome_codes_at_the_captured_probabilities():
    """ds_outcome_codes_device restates fast_custom_error as numba types it: positive iff (double)p > threshold.  Margins
    are walked across each threshold in steps of a third of a float32 step of the probability; wherever the device's own
    probability is a planted float32 (the nearest to the threshold or one of its neighbours) the code is the captured
    float64-typed verdict for that value, with both labels; beyond the neighbours it is the neighbour's verdict.  At 0.6, whose float32 lies above it, the nearest
    float32 is positive here and negative in the float32 compare of the error matrix and of predict.py."""
    import doppel_speller_amd as ds
    from doppel_speller_amd import _lib
    g = rc.OBJECTIVE
    planted = g["planted_p"]
    for i, threshold in enumerate(g["thresholds"].tolist()):
        verdict = {}
        for value, positive in zip(planted.tolist(), g["positive_f64"][i].tolist()):
            assert verdict.setdefault(value, positive) == positive                      # one verdict per float32
        step = float(np.spacing(np.float32(threshold))) / (threshold * (1 - threshold)) / 3
        margins = np.unique((np.log(threshold / (1 - threshold)) + step * np.arange(-45, 46)).astype(np.float32))
        n = margins.shape[0]
        forest = rc.margin_lookup_forest(margins)
        model = ds.ForestModel(forest["feature"], forest["threshold"], forest["yes"], forest["no"], forest["missing"],
                               forest["tree_offsets"], 1, 0.0)
        rows = (np.arange(n, dtype=np.float32) + np.float32(0.5)).reshape(-1, 1)
        assert model.predict(rows, output_margin=True).tobytes() == margins.tobytes()
        p = model.predict(rows)                                          # the device's own float32 probabilities
        around = [np.nextafter(np.float32(threshold), np.float32(0)), np.float32(threshold),
                  np.nextafter(np.float32(threshold), np.float32(1))]
        reached = [bool((p == value).any()) for value in around]
        # 1 + expf(-margin) is rounded to float32 before the division, so below 0.9 and below 0.5 the device's probability
        # skips float32 values; the nearest float32 and its upper neighbour are reached at every threshold, the lower one
        # at 0.6 and 0.7
        assert reached[1] and reached[2] and (reached[0] or threshold in (0.9, 0.5)), (threshold, reached)
        assert p.min() < around[0] and p.max() > around[2]
        d_margins = _lib.DeviceArray.from_host(margins)
        for label in (0.0, 1.0):
            d_target = _lib.DeviceArray.from_host(np.full(n, label, dtype=np.float32))
            d_codes = _lib.DeviceArray.from_host(np.full(n, 9, dtype=np.uint8))
            _lib.check(_lib.lib().ds_outcome_codes_device(d_margins.ptr, d_target.ptr, n, threshold, d_codes.ptr, None),
                       "codes")
            _sync()
            codes = d_codes.to_host()
            assert np.array_equal(codes >= 2, np.full(n, label != 0))     # 0 tn, 1 fp, 2 fn, 3 tp
            positive = (codes & 1).astype(bool) if label == 0 else codes == 3
            checked = 0
            for row in range(n):
                if float(p[row]) in verdict:
                    assert positive[row] == verdict[float(p[row])], (threshold, label, p[row])
                    checked += 1
            assert checked >= sum(reached) >= 2
            assert positive[p > around[2]].all() and not positive[p < around[0]].any()
    assert g["positive_f64"][2][planted == np.float32(0.6)].all() and not g["positive_f32"][2][planted == np.float32(0.6)].any()


# ---- end to end behind a real Jaccard stage -----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def end_to_end():
    import doppel_speller_amd as ds
    e = rc.END_TO_END
    row_of = {int(title_id): row for row, title_id in enumerate(rc.E2E_TRUTH_IDS)}
    truth_lengths = np.array([[len(rc.E2E_TRUTH_TITLES[row_of[int(i)]]) for i in ids] for ids in e["candidate_ids"]])
    forest = rc.pair_lookup_forest([len(t) for t in rc.E2E_TITLES], truth_lengths, e["margins"], float(e["default_margin"]))
    model = ds.ForestModel(forest["feature"], forest["threshold"], forest["yes"], forest["no"], forest["missing"],
                           forest["tree_offsets"], ds.FEATURES_COUNT, 0.0)
    return ds.Prediction(rc.E2E_TRUTH_TITLES, rc.E2E_TRUTH_IDS, model, top_n=int(e["top_n"]), transform=False,
                         probability_threshold=float(e["threshold"]))


def test_generate_test_predictions_reproduces_the_captured_final_table(end_to_end):
    """Jaccard top-4, exact, close, features, the lookup forest, selection and the final table on the device against what
    the reference's stage functions gave behind its own MatchMaker: the table, and which stage answered each title."""
    e = rc.END_TO_END
    p = end_to_end
    n = len(rc.E2E_TITLES)
    for chunk in (None, 1, 5):                                        # the answer of a title does not depend on its chunk
        p.chunk_queries = chunk
        out = p.generate_test_predictions(rc.E2E_TITLES)
        assert list(out.columns) == ["title_id", "test_index"]
        assert np.array_equal(out["test_index"].to_numpy(), e["final_index"]), chunk
        assert np.array_equal(out["title_id"].to_numpy(), e["final_id"]), chunk
        exact, close, model = rc.e2e_stage_ids()
        stage, title_id = p.details["stage"].to_numpy(), p.details["title_id"].to_numpy()
        for number, ids in ((1, exact), (2, close), (3, model)):
            assert np.array_equal(np.where(stage == number, title_id, rc.NOT_FOUND), ids), (chunk, number)
    p.chunk_queries = None
    assert (e["final_id"] == rc.NOT_FOUND).sum() == 6 and {0, 1, 2, 3} == set(stage.tolist())
    backwards = p.generate_test_predictions(rc.E2E_TITLES[::-1], test_index=np.arange(n)[::-1])
    assert np.array_equal(backwards["title_id"].to_numpy(), e["final_id"])
    assert np.array_equal(backwards["test_index"].to_numpy(), e["final_index"])


def test_ranked_matches_rank_1_is_the_reference_answer(end_to_end):
    """Prediction.ranked_matches on the same titles: the candidates are those of the reference's MatchMaker, and rank 1 is
    the reference's single answer wherever the reference gives one."""
    e = rc.END_TO_END
    p = end_to_end
    ranked = p.ranked_matches(rc.E2E_TITLES, n=2, keep_candidates=True)
    got = rc.E2E_TRUTH_IDS[p.candidates.rows]
    assert np.array_equal(np.sort(got, axis=1), np.sort(e["candidate_ids"], axis=1))
    first = ranked[ranked["rank"] == 1].sort_values("test_index")
    assert np.array_equal(first["test_index"].to_numpy(), np.arange(len(rc.E2E_TITLES)))
    given = e["final_id"] != rc.NOT_FOUND
    assert given.sum() == 12 and np.array_equal(first["title_id"].to_numpy()[given], e["final_id"][given])
    exact, close, _ = rc.e2e_stage_ids()
    assert np.array_equal(first["stage"].to_numpy() == 1, exact != rc.NOT_FOUND)
    assert np.array_equal(first["stage"].to_numpy() == 2, close != rc.NOT_FOUND)
