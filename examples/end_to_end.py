#!/usr/bin/env python3
"""The whole path of doppel-speller's `generate-predictions` on the GPU, from raw titles to match probabilities:

    transform_title -> MatchMaker (index build + Jaccard top-k) -> fuzzy close matches -> construct_features
                    -> tree ensemble

using only this package (reference: doppelspeller/predict.py:107-262).  Data and model are synthetic stand-ins: the
example data set and the pickled xgboost model of the reference are not part of this repository.

    python examples/end_to_end.py [n_truth] [n_queries] [top_n] [--one-to-one]

--one-to-one adds a step for linking two de-duplicated files: every truth title given to one query at most.
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import doppel_speller_amd as ds  # noqa: E402
from doppel_speller_amd import synth  # noqa: E402


def main(n_truth=20000, n_queries=2000, top_n=10, one_to_one=False):
    workload = synth.make_workload(n_truth, n_queries, seed=11)
    raw_truth = [t.upper().replace(" ", "  ") + "." for t in synth._to_strings(workload.t_flat, workload.t_off)]
    raw_queries = [t.title() for t in synth._to_strings(workload.q_flat, workload.q_off)]

    t0 = time.perf_counter()
    truth = ds.transform_titles(raw_truth)                                   # common.py:20-47
    queries = ds.transform_titles(raw_queries)
    match_maker = ds.MatchMaker.from_titles(queries, truth, top_n)           # match_maker.py:84-109 (native build)
    rows = match_maker.get_closest_matches_batch()                           # match_maker.py:192-203, every query
    t1 = time.perf_counter()

    # encoded titles + truth word counts (feature_engineering.py:298-319), uploaded once
    words = {}
    for title in truth:
        for word in set(title.split()):
            words[word] = words.get(word, 0) + 1
    t_enc, t_len = ds.encode_titles(truth)
    q_enc, q_len = ds.encode_titles(queries)
    t_counts = np.stack([ds.get_truth_words_counts(title, words) for title in truth])
    truth_table = ds.TitleTable(t_enc, t_len, t_counts)
    query_table = ds.TitleTable(q_enc, q_len)

    ratios, best_row = ds.find_close_matches(query_table, truth_table, rows)  # predict.py:140-183
    pair_q = np.repeat(np.arange(len(queries), dtype=np.int32), top_n)
    features = ds.construct_features_indexed(query_table, truth_table, pair_q, rows.reshape(-1), ds.SPACE_CODE, len(truth))
    forest = synth.make_forest(n_trees=100)
    model = ds.ForestModel(forest["feature"], forest["threshold"], forest["yes"], forest["no"], forest["missing"],
                           forest["tree_offsets"], forest["n_features"], forest["base_margin"])
    probabilities = model.predict(features).reshape(len(queries), top_n)     # predict.py:229-234
    t2 = time.perf_counter()

    found = (best_row >= 0).sum()
    print(f"{len(truth)} truth titles, {len(queries)} queries, top-{top_n}")
    print(f"index build + top-k: {t1 - t0:.2f}s   close matches + features + model: {t2 - t1:.2f}s")
    print(f"fuzzy step alone decided {found} queries; feature matrix {features.shape}; "
          f"best model score per query: mean {probabilities.max(axis=1).mean():.3f}")

    # the same question answered by the driver: one title_id (or -1) per query, every stage on the device
    ids = np.arange(len(truth), dtype=np.int64)
    prediction = ds.Prediction(raw_truth, ids, model, top_n=top_n)
    answer = prediction.generate_test_predictions(raw_queries)
    print(f"Prediction: {(answer['title_id'] >= 0).sum()} of {len(answer)} queries matched")
    # the row the model likes best over the WHOLE truth set, per title: where it was not among the Jaccard top_n
    # (jaccard_position -1) the candidate stage missed it, not the model
    best = prediction.exhaustive_matches(raw_queries, n=1)
    print(f"exhaustive rank-1 row inside the Jaccard top-{top_n}: {(best['jaccard_position'] >= 0).sum()} of {len(best)} "
          f"queries ({(best['jaccard_position'] >= 0).mean():.3f})")

    # a review queue for the titles left at -1: their best three candidates in order, with the scores
    unmatched = answer.loc[answer["title_id"] < 0, "test_index"].to_numpy()[:3]
    ranked = prediction.ranked_matches([raw_queries[i] for i in unmatched], n=min(3, top_n), test_index=unmatched)
    print(ranked.to_string(index=False))

    # how good are the answers?  The workload knows the truth title every query was made from (-1: from none): the counts
    # of the reference's get-predictions-accuracy at this instance's thresholds, then the same for a grid of both
    # thresholds from one scoring pass, and the cell with the smallest custom error
    actual = workload.actual_row                                             # ids are the truth rows here
    print("evaluate:", prediction.evaluate(raw_queries, actual))
    sweep = prediction.threshold_sweep(raw_queries, actual, levenshtein_thresholds=range(86, 100, 2),
                                       probability_thresholds=np.linspace(0.5, 0.95, 10))
    best = sweep.loc[sweep["custom_error"].idxmin()]
    print(f"smallest custom error of {len(sweep)} cells: {int(best['custom_error'])} at levenshtein_threshold "
          f"{int(best['levenshtein_threshold'])}, probability_threshold {best['probability_threshold']:.2f}")
    if one_to_one:
        # the same titles with every truth title given to one query at most: a query that loses its first choice goes on
        # to its next candidate, which may displace somebody else in turn
        linked = prediction.one_to_one_matches(raw_queries, n=min(5, top_n))
        print(f"one-to-one: {(linked['title_id'] >= 0).sum()} of {len(linked)} queries matched, no title_id twice:",
              prediction.assignment_counts)
    return rows, best_row, features, probabilities


if __name__ == "__main__":
    main(*[int(a) for a in sys.argv[1:] if a != "--one-to-one"][:3], one_to_one="--one-to-one" in sys.argv[1:])
