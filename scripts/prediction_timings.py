"""Prediction.generate_test_predictions at a bench shape with the query side prepared on the device and on the host,
and Prediction.ranked_matches (query side on the device) beside them, alternated in one process: `timings` per stage
and the whole call of every warm call, then the medians with their ranges.  The two paths must give the same answer, and
rank 1 of the ranked list must be that answer wherever there is one (checked on every call).

    python scripts/prediction_timings.py [--truth 500000] [--queries 100000] [--k 100] [--calls 3] [--ranked 5]
                                         [--out FILE]
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
    parser.add_argument("--ranked", type=int, default=5, help="slots per title of ranked_matches (0: leave it out)")
    parser.add_argument("--seed", type=int, default=20260101)
    parser.add_argument("--out", default=None, help="JSON file for the per-call timings")
    args = parser.parse_args()

    w = synth.make_workload(args.truth, args.queries, seed=args.seed)
    truth, queries = synth._to_strings(w.t_flat, w.t_off), synth._to_strings(w.q_flat, w.q_off)
    forest = synth.make_forest()
    model = ds.ForestModel(forest["feature"], forest["threshold"], forest["yes"], forest["no"], forest["missing"],
                           forest["tree_offsets"], forest["n_features"], forest["base_margin"])
    started = time.perf_counter()
    p = ds.Prediction(truth, np.asarray(w.title_id, dtype=np.int64), model, top_n=args.k)
    print(f"truth side of {args.truth} titles built in {time.perf_counter() - started:.1f} s", flush=True)

    reference = None
    calls = {"device": [], "host": []}
    if args.ranked:
        calls["ranked"] = []
    for call in range(args.calls + 1):              # call 0 of each path warms it up
        for path in calls:
            p.prepare_queries = "host" if path == "host" else "device"
            started = time.perf_counter()
            if path == "ranked":
                ranked = p.ranked_matches(queries, n=args.ranked)
            else:
                out = p.generate_test_predictions(queries)
            total = (time.perf_counter() - started) * 1000.0
            if path == "ranked":
                first = ranked[ranked["rank"] == 1].set_index("test_index")["title_id"]
                answered = reference[reference["title_id"] >= 0].set_index("test_index")["title_id"]
                assert first.loc[answered.index].equals(answered), "rank 1 is not the answer"
            else:
                if reference is None:
                    reference = out
                assert out.equals(reference), f"the {path} path gave another answer"
            if call:
                calls[path].append(dict(p.timings, call=total))
                print(path, json.dumps({name: round(ms, 2) for name, ms in calls[path][-1].items()}), flush=True)
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
