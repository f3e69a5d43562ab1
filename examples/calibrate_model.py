#!/usr/bin/env python3
"""What does the model's probability mean?  On the synthetic sets of examples/train_model.py:

    the model (model.npz of an earlier examples/train_model.py run, else one trained here with ds.train_model)
             -> the evaluation set of FeatureEngineering.generate_train_and_evaluation_data_sets
             -> ForestModel.calibrate: the isotonic fit of the labels on the model's probability, on the device
             -> the reliability of the raw probability and of the calibrated value, and the raw thresholds that stand
                for the calibrated levels 0.9, 0.95 and 0.99 (Calibrator.raw_threshold)

    python examples/calibrate_model.py [model.npz] [n_truth] [n_queries] [--bins N] [--save calibrator.npz]

The evaluation set is the one the trainer stopped on, so the calibrated table is mildly optimistic; labelled rows the
model has never seen give the honest map.  A threshold printed here is used as
Prediction(..., probability_threshold=calibrator.raw_threshold(q)).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import doppel_speller_amd as ds  # noqa: E402
from doppel_speller_amd import synth  # noqa: E402


def print_report(title, report):
    print(f"{title}: {report.n} rows in {report.n_bins} bins ({report.n_outside} outside [0, 1]); ECE {report.ece:.5f}, "
          f"MCE {report.mce:.5f}, Brier {report.brier:.6f}")
    print(report.frame().to_string(index=False, float_format=lambda value: f"{value:.4f}"))


def main(path=None, n_truth=20000, n_queries=4000, n_bins=10, save=None):
    train = synth.make_workload(n_truth, n_queries, seed=11, query_seed=101)
    truth_titles = synth._to_strings(train.t_flat, train.t_off)
    train_titles = synth._to_strings(train.q_flat, train.q_off)
    train_ids = np.where(train.actual_row >= 0, train.title_id[np.maximum(train.actual_row, 0)], -1)
    if path:
        model = ds.ForestModel.load(path)
        print(f"loaded {path}: {model.n_trees} trees")
    else:
        model = ds.train_model(truth_titles, train.title_id, train_titles, train_ids).model
        print(f"trained a model of {model.n_trees} trees (pass a model.npz to calibrate a saved one)")
    fe = ds.FeatureEngineering(truth_titles, train.title_id, train_titles, train_ids)
    _, _, evaluation, target = fe.generate_train_and_evaluation_data_sets()
    calibrator = model.calibrate(evaluation, target)
    probabilities = model.predict(evaluation)
    print(f"isotonic fit on {calibrator.n_rows} evaluation rows ({int(calibrator.pos.sum())} positive, "
          f"{calibrator.n_nan} with a NaN score): {len(calibrator)} blocks")
    print(calibrator.frame().to_string(index=False))
    raw = ds.reliability(probabilities, target, n_bins)
    calibrated = ds.reliability(calibrator.transform(probabilities), target, n_bins)
    print_report("raw probability", raw)
    print_report("calibrated value", calibrated)
    for q in (0.9, 0.95, 0.99):
        print(f"calibrated level {q}: probability_threshold = {calibrator.raw_threshold(q)!r}")
    at = calibrator.transform(np.array([0.9], np.float32))[0]
    print(f"the raw threshold 0.9 stands for an observed match rate of {at:.4f}")
    if save:
        calibrator.save(save)
        print(f"saved {save}")
    return calibrator, raw, calibrated


if __name__ == "__main__":
    arguments = sys.argv[1:]
    bins, save_path = 10, None
    if "--bins" in arguments:
        at = arguments.index("--bins")
        bins = int(arguments[at + 1])
        del arguments[at:at + 2]
    if "--save" in arguments:
        at = arguments.index("--save")
        save_path = arguments[at + 1]
        del arguments[at:at + 2]
    model_path = arguments.pop(0) if arguments and not arguments[0].isdigit() else None
    main(model_path, *[int(a) for a in arguments[:2]], n_bins=bins, save=save_path)
