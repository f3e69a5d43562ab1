"""Prediction.one_to_one_matches at a bench shape, beside Prediction.ranked_matches on the same instance and titles: the
`timings` of every stage, the counts of the matching, and the whole call of `ranked_matches` over a few warm calls (median
and range), so that the stage stands next to the pipeline it follows.

    python scripts/one_to_one_timings.py [--truth 500000] [--queries 100000] [--k 100] [--n 5] [--calls 3]
                                         [--ranked-only] [--out FILE]

--ranked-only leaves one_to_one_matches out: for a library of an earlier commit (DS_LIBRARY), to compare ranked_matches.
The synthetic forest puts no pair above the default threshold of 0.9, so the matching is run twice: at the instance's
threshold (exact and close edges only) and at the median probability of the model slots (about half of them edges).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import doppel_speller_amd as ds  # noqa: E402
from doppel_speller_amd import synth  # noqa: E402


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--truth", type=int, default=500_000)
    parser.add_argument("--queries", type=int, default=100_000)
    parser.add_argument("--k", type=int, default=100)
    parser.add_argument("--n", type=int, default=5)
    parser.add_argument("--calls", type=int, default=3, help="warm calls of ranked_matches")
    parser.add_argument("--ranked-only", action="store_true")
    parser.add_argument("--seed", type=int, default=20260101)
    parser.add_argument("--out", default=None, help="JSON file for the timings")
    args = parser.parse_args()

    w = synth.make_workload(args.truth, args.queries, seed=args.seed)
    truth, queries = synth._to_strings(w.t_flat, w.t_off), synth._to_strings(w.q_flat, w.q_off)
    forest = synth.make_forest()
    model = ds.ForestModel(forest["feature"], forest["threshold"], forest["yes"], forest["no"], forest["missing"],
                           forest["tree_offsets"], forest["n_features"], forest["base_margin"])
    started = time.perf_counter()
    p = ds.Prediction(truth, np.asarray(w.title_id, dtype=np.int64), model, top_n=args.k)
    print(f"truth side of {args.truth} titles built in {time.perf_counter() - started:.1f} s", flush=True)

    report = {"shape": vars(args), "ranked": [], "one_to_one": []}
    for call in range(args.calls + 1):                 # call 0 warms up
        started = time.perf_counter()
        ranked = p.ranked_matches(queries, n=args.n)
        total = (time.perf_counter() - started) * 1000.0
        if call:
            report["ranked"].append(dict(p.timings, call=total))
            print("ranked", json.dumps({name: round(ms, 2) for name, ms in report["ranked"][-1].items()}), flush=True)
    rows = report["ranked"]
    print("median ranked:", json.dumps({name: round(float(np.median([row[name] for row in rows])), 2) for name in rows[0]}))
    print("range ranked:", json.dumps({name: [round(min(row[name] for row in rows), 2), round(max(row[name] for row in rows), 2)]
                                        for name in rows[0]}), flush=True)
    if not args.ranked_only:
        median = float(np.median(ranked.loc[ranked["stage"] == 3, "probability"].to_numpy()))
        for threshold in (None, median):
            started = time.perf_counter()
            answer = p.one_to_one_matches(queries, n=args.n, probability_threshold=threshold)
            total = (time.perf_counter() - started) * 1000.0
            found = answer.loc[answer["title_id"] >= 0, "title_id"]
            assert not found.duplicated().any(), "a truth title was given twice"
            report["one_to_one"].append({"probability_threshold": p.probability_threshold if threshold is None else threshold,
                                         "timings": dict(p.timings, call=total), "counts": p.assignment_counts})
            print("one_to_one", json.dumps(report["one_to_one"][-1]), flush=True)
    if args.out:
        with open(args.out, "w") as handle:
            json.dump(report, handle, indent=1)


if __name__ == "__main__":
    main()
