#!/usr/bin/env python3
"""Batched cross-validation against the same boosters fitted one after another ("Cross-validation
and tuning", Measurements): a 12-set grid x 5 folds for ROUNDS rounds without early stopping.

    batch       cross_validate(x, y, grid, n_folds=5, refit=False)
    sequential  for every set and fold ForestTrainer.fit on the fold's host subset (x[train], y[train], x[held],
                y[held]): the path that exists without the batch

Three runs of each, alternated in one process after one warm-up each; prints the median and range of the totals, the
batch's boost time per round, and 60 x the single trainer's per-round time.

`single` is ForestTrainer on all rows at depth 5, the median of 10 rounds after 2: the figure of section 9's table.

    python scripts/cv_timings.py [rows] [rounds] [--batch-only] [--once] [--single-only] [--subsample=F] [--monotone]

--batch-only leaves out the sequential path, --once runs each path a single time without a warm-up (for a kernel trace),
--single-only stops after the single trainer's figure, --subsample=F adds the single trainer's figure with subsample F,
--monotone its figure with the first 17 of the 66 columns constrained upwards ("Monotone constraints").
"""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import doppel_speller_amd as ds  # noqa: E402


def data(n, nf=66, seed=3):
    rng = np.random.RandomState(seed)
    x = rng.randn(n, nf).astype(np.float32)
    y = (x[:, 0] + 0.5 * x[:, 1] * x[:, 2] + 0.5 * rng.randn(n) > 1.0).astype(np.float32)
    return x, y


def main(n=100000, rounds=100, batch_only=False, once=False, single_only=False, subsample=None, monotone=False):
    x, y = data(n)
    grid = ds.parameter_grid(max_depth=[4, 5], eta=[0.1, 0.3], beta=[1.0, 2.0, 5.0])
    folds = ds.fold_assignment(None, 5, 0, n)
    never = rounds + 1                                           # no early stopping
    subsets = None if batch_only else [(x[folds != k], y[folds != k], x[folds == k], y[folds == k]) for k in range(5)]

    def batch():
        mark = time.perf_counter()
        cv = ds.cross_validate(x, y, grid, n_folds=5, num_boost_round=rounds, early_stopping_rounds=never, refit=False)
        return time.perf_counter() - mark, cv.timings["boost"] / 1000.0

    def sequential():
        mark, boost = time.perf_counter(), 0.0
        for parameters in grid:
            for subset in subsets:
                trainer = ds.ForestTrainer().begin(*subset, **parameters)
                started = time.perf_counter()
                for _ in range(rounds):
                    trainer.step()
                boost += time.perf_counter() - started
                trainer.close()
        return time.perf_counter() - mark, boost

    def single(**sampling):
        trainer = ds.ForestTrainer().begin(x, y, x[:n // 10], y[:n // 10], **sampling)
        times = []
        for round_ in range(12):
            mark = time.perf_counter()
            trainer.step()
            times.append((time.perf_counter() - mark) * 1000.0)
        trainer.close()
        times = times[2:]
        label = "".join(f" {name}={value}" for name, value in sampling.items() if name != "monotone_constraints")
        if "monotone_constraints" in sampling:
            label += f" monotone_constraints={int(np.count_nonzero(sampling['monotone_constraints']))} columns"
        print(f"single     n={n}{label}: {statistics.median(times):.3f} ms per round ({min(times):.3f}-{max(times):.3f}), "
              f"x 60 = {statistics.median(times) * 60:.1f} ms", flush=True)

    single()
    if subsample is not None:
        single(subsample=subsample)
    if monotone:
        single(monotone_constraints=[1] * 17 + [0] * (x.shape[1] - 17))
    if single_only:
        return
    runs = {"batch": [], "sequential": []}
    paths = [("batch", batch)] + ([] if batch_only else [("sequential", sequential)])
    for name, path in paths:
        if not once:
            path()                                                # warm-up
    for _ in range(1 if once else 3):
        for name, path in paths:
            runs[name].append(path())
    for name, _ in paths:
        totals, boosts = [r[0] for r in runs[name]], [r[1] for r in runs[name]]
        print(f"{name:10s} n={n} rounds={rounds}: total median {statistics.median(totals):.3f} s "
              f"({min(totals):.3f}-{max(totals):.3f}); rounds alone median {statistics.median(boosts):.3f} s = "
              f"{statistics.median(boosts) / rounds * 1000:.2f} ms per round of 60 boosters", flush=True)


if __name__ == "__main__":
    arguments = [a for a in sys.argv[1:] if not a.startswith("--")]
    subsamples = [float(a.split("=", 1)[1]) for a in sys.argv[1:] if a.startswith("--subsample=")]
    main(*(int(a) for a in arguments[:2]), batch_only="--batch-only" in sys.argv, once="--once" in sys.argv,
         single_only="--single-only" in sys.argv, subsample=subsamples[0] if subsamples else None,
         monotone="--monotone" in sys.argv)
