"""The train-model step at a bench shape (500k truth titles, 100k train titles, top-100, 10
sampled) as the host chain (generate_train_and_evaluation_data_sets -> ForestTrainer.fit -> feature_importance ->
evaluation_error_matrix) and as train_model (the feature matrix kept in HBM), alternated in one process: one warm-up
each, then `--calls` calls each; medians and ranges per stage and for the whole call.  The two must give the same model
(checked on every call).  Then compute_cuts against compute_cuts_device at --cuts-rows rows of that feature matrix.

    python scripts/train_model_timings.py [--truth 500000] [--train 100000] [--k 100] [--calls 3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import doppel_speller_amd as ds  # noqa: E402
from doppel_speller_amd import _lib, synth  # noqa: E402

MODEL_KEYS = ("feature", "threshold", "yes", "no", "missing", "tree_offsets")


def host_chain(truth, truth_ids, train, train_ids, k, sample_n, seed):
    started = time.perf_counter()
    fe = ds.FeatureEngineering(truth, truth_ids, train, train_ids, top_n=k, sample_n=sample_n, seed=seed)
    features, labels, eval_features, eval_labels = fe.generate_train_and_evaluation_data_sets()
    timings = dict(fe.timings)
    mark = time.perf_counter()
    cuts = ds.compute_cuts(features)
    timings["cuts"] = (time.perf_counter() - mark) * 1000.0      # measured apart: fit computes them again inside
    mark = time.perf_counter()
    trainer = ds.ForestTrainer()
    model = trainer.fit(features, labels, eval_features, eval_labels)
    timings["fit"] = (time.perf_counter() - mark) * 1000.0
    mark = time.perf_counter()
    importance = model.feature_importance()
    matrix = ds.evaluation_error_matrix(model, eval_features, eval_labels)
    timings["evaluate"] = (time.perf_counter() - mark) * 1000.0
    timings["total"] = (time.perf_counter() - started) * 1000.0 - timings["cuts"]
    del cuts
    return model, importance, matrix, trainer.best_iteration, timings, fe


def summary(rows):
    return {name: [round(float(np.median([row[name] for row in rows])), 1),
                   round(float(min(row[name] for row in rows)), 1), round(float(max(row[name] for row in rows)), 1)]
            for name in rows[0]}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--truth", type=int, default=500_000)
    parser.add_argument("--train", type=int, default=100_000)
    parser.add_argument("--k", type=int, default=100)
    parser.add_argument("--sample", type=int, default=10)
    parser.add_argument("--calls", type=int, default=3, help="timed calls per chain, after one warm-up each")
    parser.add_argument("--seed", type=int, default=20260101)
    parser.add_argument("--cuts-rows", type=int, nargs="*", default=[1_000_000, 10_000_000])
    parser.add_argument("--out", default=None, help="JSON file for the per-call timings")
    args = parser.parse_args()

    w = synth.make_workload(args.truth, args.train, seed=args.seed)
    truth, train = synth._to_strings(w.t_flat, w.t_off), synth._to_strings(w.q_flat, w.q_off)
    truth_ids = np.asarray(w.title_id, dtype=np.int64)
    train_ids = np.where(w.actual_row >= 0, truth_ids[np.maximum(w.actual_row, 0)], -1)

    calls = {"host": [], "device": []}
    features = None
    for call in range(args.calls + 1):               # call 0 of each chain warms it up
        model, importance, matrix, best, timings, fe = host_chain(truth, truth_ids, train, train_ids, args.k,
                                                                  args.sample, args.seed)
        features = fe.features
        started = time.perf_counter()
        result = ds.train_model(truth, truth_ids, train, train_ids, top_n=args.k, sample_n=args.sample, seed=args.seed)
        wall = (time.perf_counter() - started) * 1000.0
        for key in MODEL_KEYS:
            assert result.model.arrays[key].tobytes() == model.arrays[key].tobytes(), f"the chains differ in {key}"
        assert result.error_matrix == matrix and result.best_iteration == best
        assert result.feature_importance.tobytes() == importance.tobytes()
        if call:
            calls["host"].append(timings)
            calls["device"].append(dict(result.timings, total=wall))
            for chain in ("host", "device"):
                print(chain, json.dumps({name: round(ms, 1) for name, ms in calls[chain][-1].items()}), flush=True)
        else:
            print(f"{fe.rows.shape[0]} rows of {features.shape[1]} features, {model.n_trees} trees, best round {best}, "
                  f"error matrix {matrix}", flush=True)
    medians = {chain: summary(rows) for chain, rows in calls.items()}
    for chain in ("host", "device"):
        print(f"median [min, max] ms {chain}:", json.dumps(medians[chain]), flush=True)
    host_total, device_total = medians["host"]["total"][0], medians["device"]["total"][0]
    print(f"whole call: host chain {host_total} ms, train_model {device_total} ms, "
          f"{host_total - device_total:.1f} ms less", flush=True)

    cuts_rows = {}
    for rows in args.cuts_rows:
        matrix = np.ascontiguousarray(np.resize(features, (rows, features.shape[1])))
        d_matrix = _lib.DeviceArray.from_host(matrix)
        host_ms, device_ms = [], []
        for repeat in range(4):                      # the first of each warms up
            mark = time.perf_counter()
            want = ds.compute_cuts(matrix)
            host_ms.append((time.perf_counter() - mark) * 1000.0)
            mark = time.perf_counter()
            got = ds.compute_cuts_device(d_matrix, rows)
            device_ms.append((time.perf_counter() - mark) * 1000.0)
            assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
        d_matrix.free()
        cuts_rows[rows] = {"host": summary([{"ms": v} for v in host_ms[1:]])["ms"],
                           "device": summary([{"ms": v} for v in device_ms[1:]])["ms"]}
        print(f"cuts of {rows} rows, median [min, max] ms:", json.dumps(cuts_rows[rows]), flush=True)
    assert device_total < host_total, "train_model was not faster than the host chain"
    if args.out:
        with open(args.out, "w") as handle:
            json.dump({"shape": vars(args), "calls": calls, "medians": medians, "cuts": cuts_rows}, handle, indent=1)


if __name__ == "__main__":
    main()
