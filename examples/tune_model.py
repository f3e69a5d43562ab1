#!/usr/bin/env python3
"""Which booster parameters, and how many rounds?  A small grid cross-validated on synthetic titles:

    truth titles + train titles with their ids (-1: made up)
             -> tune_model_parameters: the training set in HBM (FeatureEngineering without an evaluation split), folds
                by train title, K folds x P parameter sets boosted together on the device, the best set refit on all rows

It prints the `results` table (one line per parameter set: the out-of-fold custom error at its best round), the chosen
set and the stages' times.

    python examples/tune_model.py [n_truth] [n_queries] [n_folds]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import doppel_speller_amd as ds  # noqa: E402
from doppel_speller_amd import synth  # noqa: E402


def main(n_truth=20000, n_queries=4000, n_folds=5):
    w = synth.make_workload(n_truth, n_queries, seed=11, query_seed=101)
    truth_titles = synth._to_strings(w.t_flat, w.t_off)
    train_titles = synth._to_strings(w.q_flat, w.q_off)
    train_ids = np.where(w.actual_row >= 0, w.title_id[np.maximum(w.actual_row, 0)], -1)
    grid = ds.parameter_grid(max_depth=[3, 5], eta=[0.1, 0.3], beta=[2.0, 5.0])
    tuned = ds.tune_model_parameters(truth_titles, w.title_id, train_titles, train_ids, grid, n_folds=n_folds,
                                     transform=False, num_boost_round=300, early_stopping_rounds=30)
    print(tuned.results.to_string())
    print(f"{len(tuned.rows)} rows, {n_folds} folds x {len(grid)} sets; chosen: {tuned.best_parameters}, "
          f"{tuned.best_iteration + 1} trees, out-of-fold error {tuned.results['error'][tuned.chosen]}")
    print("ms:", {stage: round(ms, 1) for stage, ms in tuned.timings.items()})
    return tuned


if __name__ == "__main__":
    main(*(int(argument) for argument in sys.argv[1:4]))
