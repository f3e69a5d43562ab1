"""Prediction.threshold_sweep at a bench shape on a 20 x 50 grid and on one cell, beside generate_test_predictions and
ranked_matches(n=1) of the same build, alternated in one process: `timings` per stage and the whole call of every warm
call, then the medians with their ranges.  The sweep's line at the instance's own thresholds must be
predictions_accuracy of what generate_test_predictions answers (checked on every call).

    python scripts/sweep_timings.py [--truth 500000] [--queries 100000] [--k 100] [--calls 3] [--out FILE]
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
    parser.add_argument("--calls", type=int, default=3, help="warm calls per path")
    parser.add_argument("--seed", type=int, default=20260101)
    parser.add_argument("--out", default=None, help="JSON file for the per-call timings")
    args = parser.parse_args()

    w = synth.make_workload(args.truth, args.queries, seed=args.seed)
    truth, queries = synth._to_strings(w.t_flat, w.t_off), synth._to_strings(w.q_flat, w.q_off)
    ids = np.asarray(w.title_id, dtype=np.int64)
    actual = np.where(w.actual_row >= 0, ids[np.maximum(w.actual_row, 0)], -1)
    forest = synth.make_forest()
    model = ds.ForestModel(forest["feature"], forest["threshold"], forest["yes"], forest["no"], forest["missing"],
                           forest["tree_offsets"], forest["n_features"], forest["base_margin"])
    started = time.perf_counter()
    p = ds.Prediction(truth, ids, model, top_n=args.k)
    print(f"truth side of {args.truth} titles built in {time.perf_counter() - started:.1f} s", flush=True)

    grids = {"sweep_20x50": (sorted({p.levenshtein_threshold, *range(81, 101)}),
                             sorted({p.probability_threshold, *np.linspace(0.5, 0.99, 49).tolist()})),
             "sweep_1x1": (None, None)}
    calls = {"predictions": [], "ranked_1": [], "sweep_1x1": [], "sweep_20x50": []}      # the grid last: its frame is kept
    expected = None
    for call in range(args.calls + 1):              # call 0 of each path warms it up
        for path in calls:
            started = time.perf_counter()
            if path == "predictions":
                answer = p.generate_test_predictions(queries)
            elif path == "ranked_1":
                p.ranked_matches(queries, n=1)
            else:
                frame = p.threshold_sweep(queries, actual, *grids[path])
            total = (time.perf_counter() - started) * 1000.0
            if path == "predictions":
                expected = ds.predictions_accuracy(answer["title_id"].to_numpy(), actual)
            elif path.startswith("sweep"):
                line = frame[(frame["levenshtein_threshold"] == p.levenshtein_threshold) &
                             (frame["probability_threshold"] == p.probability_threshold)].iloc[0]
                assert {name: int(line[name]) for name in expected} == expected, f"{path}: {dict(line)} != {expected}"
            if call:
                calls[path].append(dict(p.timings, call=total))
                print(path, json.dumps({name: round(ms, 2) for name, ms in calls[path][-1].items()}), flush=True)
    print("accuracy at the instance's thresholds:", json.dumps(expected), flush=True)
    best = frame.sort_values("custom_error", kind="stable").iloc[0]
    print("best cell of the grid:", json.dumps({name: float(best[name]) for name in frame.columns}), flush=True)
    for path, rows in calls.items():
        medians = {name: round(float(np.median([row[name] for row in rows])), 2) for name in rows[0]}
        ranges = {name: [round(min(row[name] for row in rows), 2), round(max(row[name] for row in rows), 2)]
                  for name in rows[0]}
        print(f"median {path}:", json.dumps(medians), flush=True)
        print(f"range {path}:", json.dumps(ranges), flush=True)
    if args.out:
        with open(args.out, "w") as handle:
            json.dump({"shape": vars(args), "calls": calls}, handle, indent=1)


if __name__ == "__main__":
    main()
