"""The isotonic fit at the size of examples/train_model.py ("Calibration").  A model trained on
its synthetic titles scores the evaluation rows; ds.fit_isotonic_device is timed on three inputs that lie in HBM, each
the median [min, max] of --repeats calls after one warm-up, by the host clock around a call that ends with the blocks
on the host, next to tests/calibration_oracle.py (NumPy and Python integers) on the same inputs:

    evaluation   the model's probabilities of the evaluation set against its labels
    tiled        those scores and labels repeated to 2^20 rows
    shuffled     2^20 distinct scores in random order against random labels: nothing pools at the first level but by
                 chance, so about half the points reach the serial level

The device's blocks equal the oracle's (checked).  With --serial the fit is also timed at "segment_points" 2048, 1024
(the default) and 64 in one process, alternated: the first level is parallel and the last is one thread, so what the
call loses as the segments shrink is the serial level's.  Then the two reliability tables, ECE raw against calibrated
and raw_threshold(0.9 / 0.95 / 0.99) of that model.

    python scripts/calibration_timings.py [--truth 20000] [--train 4000] [--repeats 5] [--serial] [--inputs NAME ...]

--inputs keeps the named inputs only (a kernel trace of one input: rocprofv3 --kernel-trace --stats -- python ...).
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import calibration_oracle as oracle  # noqa: E402
import doppel_speller_amd as ds  # noqa: E402
from doppel_speller_amd import _lib, calibration, synth  # noqa: E402


def timed(call, repeats):
    call()
    ms = []
    for _ in range(repeats):
        mark = time.perf_counter()
        out = call()
        ms.append((time.perf_counter() - mark) * 1000.0)
    return out, f"{np.median(ms):.2f} ms [{min(ms):.2f}, {max(ms):.2f}]"


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--truth", type=int, default=20000)
    parser.add_argument("--train", type=int, default=4000)
    parser.add_argument("--repeats", type=int, default=5)
    parser.add_argument("--serial", action="store_true")
    parser.add_argument("--inputs", nargs="*", default=["evaluation", "tiled", "shuffled"])
    args = parser.parse_args()
    w = synth.make_workload(args.truth, args.train, seed=11, query_seed=101)
    truth, train = synth._to_strings(w.t_flat, w.t_off), synth._to_strings(w.q_flat, w.q_off)
    ids = np.where(w.actual_row >= 0, w.title_id[np.maximum(w.actual_row, 0)], -1)
    model = ds.train_model(truth, w.title_id, train, ids).model
    fe = ds.FeatureEngineering(truth, w.title_id, train, ids)
    _, _, evaluation, target = fe.generate_train_and_evaluation_data_sets()
    target = np.ascontiguousarray(target, dtype=np.float32)
    probabilities = model.predict(evaluation)
    rng = np.random.default_rng(5)
    big = 1 << 20
    repeat = -(-big // probabilities.shape[0])
    inputs = {"evaluation": (probabilities, target),
              "tiled": (np.tile(probabilities, repeat)[:big], np.tile(target, repeat)[:big]),
              "shuffled": (rng.permutation(big).astype(np.float32) / np.float32(big),
                           (rng.random(big) < 0.5).astype(np.float32))}
    for name, (scores, labels) in inputs.items():
        if name not in args.inputs:
            continue
        n = scores.shape[0]
        d_scores, d_labels = _lib.DeviceArray.from_host(scores), _lib.DeviceArray.from_host(labels)
        fit, device_ms = timed(lambda: ds.fit_isotonic_device(d_scores, n, d_labels, details=True), args.repeats)
        want, oracle_ms = timed(lambda: oracle.fit(scores, labels), min(args.repeats, 2))
        got = fit.calibrator
        assert got == ds.Calibrator(want["lo"], want["hi"], want["pos"], want["neg"], want["n_nan"]), name
        print(f"{name:<11} {n} rows, {fit.n_points} points, {fit.n_serial} blocks into the serial level, {fit.n_blocks} "
              f"blocks: fit_isotonic_device {device_ms}   tests/calibration_oracle.py {oracle_ms}")
        if args.serial:
            ms = {2048: [], 1024: [], 64: []}
            for call in range(len(ms) * (args.repeats + 1)):
                width = list(ms)[call % len(ms)]
                calibration.calibrate_option("segment_points", width)
                mark = time.perf_counter()
                other = ds.fit_isotonic_device(d_scores, n, d_labels, details=True)
                if call >= len(ms):
                    ms[width].append((time.perf_counter() - mark) * 1000.0)
                assert other.calibrator == got
                serial = other.n_serial
                if call < len(ms):
                    print(f"{'':<11} segment_points {width}: {serial} blocks into the serial level")
            calibration.calibrate_option("segment_points", 0)
            print(f"{'':<11} " + ", ".join(f"segment_points {width}: {np.median(v):.2f} ms [{min(v):.2f}, {max(v):.2f}]"
                                          for width, v in ms.items()))
        d_scores.free()
        d_labels.free()
    calibrator = model.calibrate(evaluation, target)
    raw = ds.reliability(probabilities, target, 10)
    calibrated = ds.reliability(calibrator.transform(probabilities), target, 10)
    for title, report in (("raw probability", raw), ("calibrated value", calibrated)):
        print(f"{title}: ECE {report.ece:.5f}, MCE {report.mce:.5f}, Brier {report.brier:.6f}, {report.n} rows")
        print(report.frame().to_string(index=False, float_format=lambda value: f"{value:.4f}"))
    print(f"{len(calibrator)} blocks; " + ", ".join(f"raw_threshold({q}) = {calibrator.raw_threshold(q)!r}"
                                                    for q in (0.9, 0.95, 0.99)))
    print(f"the raw 0.9 maps to {calibrator.transform(np.array([0.9], np.float32))[0]:.4f}; rows above it: "
          f"{int((probabilities > 0.9).sum())}, of them positive {int(((probabilities > 0.9) & (target != 0)).sum())}")


if __name__ == "__main__":
    main()
