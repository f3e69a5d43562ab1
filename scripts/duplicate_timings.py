"""Prediction.duplicate_groups at a bench shape, with and without the model's links: `timings` per stage and the whole
call of every warm call, then the medians with their ranges, the link counters and the sizes of the groups.

    python scripts/duplicate_timings.py [--truth 500000] [--k 100] [--calls 3] [--chunk N] [--out FILE]
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
    parser.add_argument("--k", type=int, default=100)
    parser.add_argument("--calls", type=int, default=3, help="warm calls per form")
    parser.add_argument("--chunk", type=int, default=None, help="chunk_queries (default: what the free HBM suggests)")
    parser.add_argument("--seed", type=int, default=20260101)
    parser.add_argument("--out", default=None, help="JSON file for the per-call timings")
    args = parser.parse_args()

    w = synth.make_workload(args.truth, 16, seed=args.seed)
    truth = synth._to_strings(w.t_flat, w.t_off)
    forest = synth.make_forest()
    model = ds.ForestModel(forest["feature"], forest["threshold"], forest["yes"], forest["no"], forest["missing"],
                           forest["tree_offsets"], forest["n_features"], forest["base_margin"])
    started = time.perf_counter()
    p = ds.Prediction(truth, np.asarray(w.title_id, dtype=np.int64), model, top_n=args.k, chunk_queries=args.chunk)
    print(f"truth side of {args.truth} titles built in {time.perf_counter() - started:.1f} s", flush=True)

    calls = {"model_links": [], "no_model": []}
    frames = {}
    for call in range(args.calls + 1):              # call 0 of each form warms it up
        for form in calls:
            started = time.perf_counter()
            frame = p.duplicate_groups(model_links=form == "model_links")
            total = (time.perf_counter() - started) * 1000.0
            assert form not in frames or frame.equals(frames[form][0]), f"{form}: another answer on call {call}"
            frames[form] = (frame, dict(p.link_counts))
            if call:
                calls[form].append(dict(p.timings, call=total))
                print(form, json.dumps({name: round(ms, 2) for name, ms in calls[form][-1].items()}), flush=True)
    for form, rows in calls.items():
        medians = {name: round(float(np.median([row[name] for row in rows])), 2) for name in rows[0]}
        ranges = {name: [round(min(row[name] for row in rows), 2), round(max(row[name] for row in rows), 2)]
                  for name in rows[0]}
        frame, counts = frames[form]
        sizes = frame.drop_duplicates("group_id")["group_size"]
        print(f"median {form}:", json.dumps(medians), flush=True)
        print(f"range {form}:", json.dumps(ranges), flush=True)
        print(f"groups {form}:", json.dumps({"links": counts, "rows": len(frame), "groups": len(sizes),
                                             "largest": int(sizes.max()) if len(sizes) else 0}), flush=True)
    if args.out:
        with open(args.out, "w") as handle:
            json.dump({"shape": vars(args), "calls": calls}, handle, indent=1)


if __name__ == "__main__":
    main()
