"""`Prediction.timings` of every entry point on the GPU, with the query side prepared on the device and on the host: the
key set is the documented one, every device stage took time after a call with titles (three chunks, the last one ragged),
and a call without titles leaves the same keys at 0.0."""
import numpy as np
import pytest

import contributions_cases as cc

pytestmark = pytest.mark.gpu

HOST_KEYS = ("host_prepare", "copy_back")            # wall clock of the host; every other key is a device stage
PREDICT = ("host_prepare", "top_k", "close_matches", "exact_matches", "remaining_pairs", "features", "model",
           "select_matches", "copy_back")
RANKED = ("host_prepare", "top_k", "close_matches", "exact_matches", "features", "model", "rank", "copy_back")
SWEEP = ("host_prepare", "top_k", "close_parts", "exact_matches", "features", "model", "sweep", "copy_back")
KEYS = {"generate_test_predictions": PREDICT,
        "ranked_matches": RANKED,
        "one_to_one_matches": RANKED + ("assign_edges", "assign"),
        "exhaustive_matches": ("host_prepare", "top_k", "exhaustive", "copy_back"),
        "explain": ("host_prepare", "top_k", "close_matches", "exact_matches", "features", "model", "contributions",
                    "copy_back"),
        "threshold_sweep": SWEEP,
        "evaluate": SWEEP}
DUPLICATES = ("host_prepare", "prepare_queries", "top_k", "close_matches", "exact_matches", "features", "model", "links",
              "finish", "copy_back")
CALLS = {"generate_test_predictions": lambda p, titles, actual: p.generate_test_predictions(titles),
         "ranked_matches": lambda p, titles, actual: p.ranked_matches(titles, n=3),
         "one_to_one_matches": lambda p, titles, actual: p.one_to_one_matches(titles, n=3),
         "exhaustive_matches": lambda p, titles, actual: p.exhaustive_matches(titles, n=3),
         "explain": lambda p, titles, actual: p.explain(titles),
         "threshold_sweep": lambda p, titles, actual: p.threshold_sweep(titles, actual, [80, 90], [0.5, 0.9]),
         "evaluate": lambda p, titles, actual: p.evaluate(titles, actual)}


@pytest.fixture(scope="module")
def problem():
    """300 truth titles, 40 titles in chunks of 16, the top 8 candidates, 40 random trees with a counted cover; the
    first title that reaches the model stage."""
    import doppel_speller_amd as ds
    from doppel_speller_amd import synth
    w = synth.make_workload(300, 40, seed=51)
    truth, titles = synth._to_strings(w.t_flat, w.t_off), synth._to_strings(w.q_flat, w.q_off)
    ids = np.asarray(w.title_id, dtype=np.int64)
    actual = np.where(w.actual_row >= 0, ids[np.maximum(w.actual_row, 0)], -1)
    forest = synth.make_forest(seed=52, n_trees=40)
    model = ds.ForestModel(forest["feature"], forest["threshold"], forest["yes"], forest["no"], forest["missing"],
                           forest["tree_offsets"], forest["n_features"], forest["base_margin"])
    model.fit_cover(cc.random_rows(53, 4000), prior=1.0)
    p = ds.Prediction(truth, ids, model, top_n=8, transform=False, chunk_queries=16)
    p.generate_test_predictions(titles)
    late = np.nonzero(~np.isin(p.details["stage"].to_numpy(), (ds.prediction.STAGE_EXACT, ds.prediction.STAGE_CLOSE)))[0]
    assert late.shape[0], "no title reaches the model stage"
    return p, titles, actual, titles[int(late[0])]


def _keys(listed, mode, always_prepares=False):
    return set(listed) | ({"prepare_queries"} if mode == "device" or always_prepares else set())


def _check(timings, expected, zero=()):
    print(timings)
    assert set(timings) == expected
    for name, ms in timings.items():
        if name in zero:
            assert ms == 0.0, name
        elif name not in HOST_KEYS:
            assert ms > 0, name


@pytest.mark.parametrize("mode", ["device", "host"])
@pytest.mark.parametrize("entry", sorted(KEYS))
def test_keys_and_stage_times_of_an_entry_point(problem, entry, mode):
    p, titles, actual, _ = problem
    p.prepare_queries = mode
    expected = _keys(KEYS[entry], mode)
    CALLS[entry](p, titles, actual)
    _check(p.timings, expected)
    CALLS[entry](p, [], actual[:0])
    _check(p.timings, expected, zero=expected)


@pytest.mark.parametrize("mode", ["device", "host"])
def test_keys_and_stage_times_of_one_exhaustive_title(problem, mode):
    p, _, _, title = problem
    p.prepare_queries = mode
    p.closest_search_single_title(title, exhaustive=True)
    _check(p.timings, _keys(PREDICT + ("exhaustive",), mode))


@pytest.mark.parametrize("mode", ["device", "host"])
def test_keys_and_stage_times_of_duplicate_groups(problem, mode):
    p = problem[0]
    p.prepare_queries = mode
    expected = _keys(DUPLICATES, mode, always_prepares=True)
    p.duplicate_groups(return_links=True)
    _check(p.timings, expected)
    p.duplicate_groups(model_links=False)
    _check(p.timings, expected, zero=("features", "model"))
