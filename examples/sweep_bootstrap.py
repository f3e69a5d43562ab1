#!/usr/bin/env python3
"""Is the best cell of a threshold sweep really better?  On the synthetic sets of examples/train_model.py:

    the model (model.npz of an earlier examples/train_model.py run, else one trained here with ds.train_model)
             -> Prediction.threshold_sweep over the evaluation titles, a grid of 20 Levenshtein x 50 probability
                thresholds, n_boot replicates: every title scored once, one 16-bit record per (title, Levenshtein
                threshold), then one device call resamples the titles for all 1000 cells with the same draws
             -> the ten cells with the smallest error with their intervals and how often each is the best one
                (SweepBootstrap.frame), and the best cell against the defaults (94, 0.9) (SweepBootstrap.against)

    python examples/sweep_bootstrap.py [model.npz] [n_truth] [n_queries] [--n-boot N] [--seed S]

A difference whose interval holds 0, or a best cell that wins a small share of the replicates, says that another sample
of labelled titles could pick another cell: keep the defaults.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import doppel_speller_amd as ds  # noqa: E402
from doppel_speller_amd import synth  # noqa: E402

LEVENSHTEIN = list(range(81, 101))                        # 20
PROBABILITY = [round(0.5 + 0.01 * i, 2) for i in range(50)]   # 50, 0.9 among them


def main(path=None, n_truth=20000, n_queries=4000, n_boot=2000, seed=0):
    train = synth.make_workload(n_truth, n_queries, seed=11, query_seed=101)
    evaluation = synth.make_workload(n_truth, n_queries // 4, seed=11, query_seed=102)
    truth_titles = synth._to_strings(train.t_flat, train.t_off)
    if path:
        model = ds.ForestModel.load(path)
        print(f"loaded {path}: {model.n_trees} trees")
    else:
        train_ids = np.where(train.actual_row >= 0, train.title_id[np.maximum(train.actual_row, 0)], -1)
        model = ds.train_model(truth_titles, train.title_id, synth._to_strings(train.q_flat, train.q_off), train_ids).model
        print(f"trained a model of {model.n_trees} trees (pass a model.npz to sweep a saved one)")
    titles = synth._to_strings(evaluation.q_flat, evaluation.q_off)
    actual = np.where(evaluation.actual_row >= 0, evaluation.title_id[np.maximum(evaluation.actual_row, 0)], -1)
    p = ds.Prediction(truth_titles, train.title_id, model)
    p.threshold_sweep(titles, actual, LEVENSHTEIN, PROBABILITY, n_boot=n_boot, seed=seed)
    boot = p.sweep_bootstrap
    stages = ", ".join(f"{name} {p.timings[name]:.2f} ms" for name in ("sweep", "sweep_records", "sweep_bootstrap"))
    print(f"{len(titles)} titles, {len(LEVENSHTEIN)} x {len(PROBABILITY)} cells, {boot.n_boot} replicates: {stages}")
    frame = boot.frame()
    print(frame.sort_values(["custom_error", "levenshtein_threshold", "probability_threshold"]).head(10)[
        ["levenshtein_threshold", "probability_threshold", "custom_error", "mean_error", "low", "high", "share_best"]
    ].to_string(index=False, float_format=lambda value: f"{value:.3f}"))
    best, default = boot.best(), boot.cell(94, 0.9)
    line = boot.against(default).iloc[best]
    print(f"best cell {boot.names[best]} against the defaults {boot.names[default]}: difference {line['baseline']:+.0f} "
          f"(mean {line['mean']:+.1f}, 95 % interval [{line['low']:+.1f}, {line['high']:+.1f}]), better in "
          f"{100 * line['share_better']:.1f} % of the replicates; it is the best cell in {100 * boot.share_best[best]:.1f} % "
          f"of them, the defaults in {100 * boot.share_best[default]:.1f} %")
    return boot


if __name__ == "__main__":
    arguments = sys.argv[1:]
    options = {"--n-boot": 2000, "--seed": 0}
    for name in options:
        if name in arguments:
            at = arguments.index(name)
            options[name] = int(arguments[at + 1])
            del arguments[at:at + 2]
    model_path = arguments.pop(0) if arguments and not arguments[0].isdigit() else None
    main(model_path, *[int(a) for a in arguments[:2]], n_boot=options["--n-boot"], seed=options["--seed"])
