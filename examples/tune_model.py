#!/usr/bin/env python3
"""Which booster parameters, and how many rounds?  A small grid cross-validated on synthetic titles:

    truth titles + train titles with their ids (-1: made up)
             -> tune_model_parameters: the training set in HBM (FeatureEngineering without an evaluation split), folds
                by train title, K folds x P parameter sets boosted together on the device, the best set refit on all rows

It prints the `results` table (one line per parameter set: the out-of-fold custom error at its best round), the chosen
set and the stages' times.

    python examples/tune_model.py [--subsample 0.5,1] [--colsample-bytree 0.5,1] [--metrics auc,logloss]
                                  [--select-by auc] [--init-model PATH] [--monotone ratios]
                                  [n_truth] [n_queries] [n_folds]

--subsample and --colsample-bytree take comma-separated fractions in (0, 1] and add them to the grid as further axes
(row and column subsampling, ForestTrainer's parameters of those names); without them the grid is the plain one.
--metrics adds the pooled out-of-fold AUC and / or weighted log loss of every set to the table, computed on the device
in every round; --select-by error|auc|logloss names the curve that the rounds are stopped and the set is chosen on
(error, the default, is xgb.cv's rule on the custom error; auc and logloss tell apart sets whose integer errors tie).
--init-model PATH starts every fold of every set, and the refit, from the ForestModel saved at PATH (for instance
examples/train_model.py's model.npz): the table counts the NEW rounds, and its `initial_error` column is the init
model's own out-of-fold error, the baseline that continuing has to beat.
--monotone ratios constrains the 17 similarity ratios upwards in every fold, set and the refit (ds.ratio_constraints());
--monotone title_ratio=1,word_1_best_ratio=1 names columns of ds.FEATURE_NAMES and their signs.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import doppel_speller_amd as ds  # noqa: E402
from doppel_speller_amd import synth  # noqa: E402


def main(n_truth=20000, n_queries=4000, n_folds=5, subsample=None, colsample_bytree=None, metrics=(),
         select_by="error", init_model=None, monotone=None):
    init = ds.ForestModel.load(init_model) if init_model else None
    w = synth.make_workload(n_truth, n_queries, seed=11, query_seed=101)
    truth_titles = synth._to_strings(w.t_flat, w.t_off)
    train_titles = synth._to_strings(w.q_flat, w.q_off)
    train_ids = np.where(w.actual_row >= 0, w.title_id[np.maximum(w.actual_row, 0)], -1)
    sampling = {name: values for name, values in (("subsample", subsample), ("colsample_bytree", colsample_bytree))
                if values}
    grid = ds.parameter_grid(max_depth=[3, 5], eta=[0.1, 0.3], beta=[2.0, 5.0], **sampling)
    tuned = ds.tune_model_parameters(truth_titles, w.title_id, train_titles, train_ids, grid, n_folds=n_folds,
                                     transform=False, num_boost_round=300, early_stopping_rounds=30,
                                     metrics=tuple(metrics), select_by=select_by, init_model=init,
                                     monotone_constraints=monotone)
    print(tuned.results.to_string())
    print(f"{len(tuned.rows)} rows, {n_folds} folds x {len(grid)} sets; chosen: {tuned.best_parameters}, "
          f"{tuned.best_iteration + 1} trees"
          + (f" after the init model's {init.n_trees} (its out-of-fold error: {tuned.initial_errors[tuned.chosen]})"
             if init else "")
          + f", out-of-fold error {tuned.results['error'][tuned.chosen]}"
          + "".join(f", {name} {tuned.results[name][tuned.chosen]:.6f}" for name in metrics)
          + (f" (chosen by {select_by})" if select_by != "error" else ""))
    if monotone is not None:
        vector = ds.validate_monotone_constraints(monotone, ds.FEATURES_COUNT, ds.FEATURE_NAMES)
        print(f"monotone constraints on {int(np.count_nonzero(vector))} features: "
              f"{tuned.model.monotone_violations(vector)} splits of the refit model break them")
    print("ms:", {stage: round(ms, 1) for stage, ms in tuned.timings.items()})
    return tuned


def _arguments(argv):
    """(positional arguments, {option: its value}) of the command line."""
    positional, options = [], {}
    argv = list(argv)
    while argv:
        argument = argv.pop(0)
        if argument in ("--subsample", "--colsample-bytree"):
            if not argv:
                raise SystemExit(f"{argument} needs a comma-separated list of fractions")
            options[argument[2:].replace("-", "_")] = [float(value) for value in argv.pop(0).split(",")]
        elif argument in ("--metrics", "--select-by", "--init-model"):
            if not argv:
                raise SystemExit(f"{argument} needs a value")
            value = argv.pop(0)
            options[argument[2:].replace("-", "_")] = tuple(value.split(",")) if argument == "--metrics" else value
        elif argument == "--monotone":
            if not argv:
                raise SystemExit("--monotone needs `ratios` or NAME=SIGN,... over ds.FEATURE_NAMES")
            value = argv.pop(0)
            options["monotone"] = ds.ratio_constraints() if value == "ratios" else \
                {name: int(sign) for name, sign in (pair.split("=") for pair in value.split(","))}
        else:
            positional.append(int(argument))
    return positional, options


if __name__ == "__main__":
    numbers, lists = _arguments(sys.argv[1:])
    main(*numbers[:3], **lists)
