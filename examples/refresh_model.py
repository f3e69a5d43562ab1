#!/usr/bin/env python3
"""Refresh a trained match model on new data and keep its splits, on the GPU and on synthetic data:

    the training and evaluation sets of examples/train_model.py, kept in HBM (generate_device_data_sets)
             -> ForestTrainer.fit_device, or --model model.npz (a ForestModel saved by examples/train_model.py)
             -> ForestModel.refresh_device on the same matrix and parameters: the model comes back bit for bit
             -> ds.refresh_model on a second draw of train titles (another query seed): every split stays, the leaves
                follow the new rows; the evaluation custom error of the model as given next to the refreshed model's
             -> cover, gain and RefreshResult.gain_importance() next to ForestModel.feature_importance()

It prints the time of refresh_device for the model's tree count next to fit_device for the same number of rounds on the
same matrix (one process, alternating, after a warm call of each; --timed repetitions).

    python examples/refresh_model.py [--model model.npz] [--timed 5] [n_truth] [n_queries]
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import doppel_speller_amd as ds  # noqa: E402
from doppel_speller_amd import synth  # noqa: E402


def titles_of(workload):
    ids = np.where(workload.actual_row >= 0, workload.title_id[np.maximum(workload.actual_row, 0)], -1)
    return synth._to_strings(workload.q_flat, workload.q_off), ids


def main(n_truth=20000, n_queries=4000, model_path=None, repetitions=5):
    first = synth.make_workload(n_truth, n_queries, seed=11, query_seed=101)
    second = synth.make_workload(n_truth, n_queries, seed=11, query_seed=104)
    truth_titles = synth._to_strings(first.t_flat, first.t_off)
    train_titles, train_ids = titles_of(first)
    fe = ds.FeatureEngineering(truth_titles, first.title_id, train_titles, train_ids)
    sets = fe.generate_device_data_sets()
    data = (sets.train, sets.n_train, sets.train_target, sets.evaluation, sets.n_evaluation, sets.evaluation_target)
    trainer = ds.ForestTrainer()
    if model_path:
        model = ds.ForestModel.load(model_path)
    else:
        model = trainer.fit_device(*data)
    print(f"model: {model.n_trees} trees, {model.n_nodes} nodes; training set {sets.n_train} rows, evaluation set "
          f"{sets.n_evaluation} rows")

    same = model.refresh_device(*data)
    identical = same.model.arrays["threshold"].tobytes() == model.arrays["threshold"].tobytes()
    print(f"refreshed on its own training set: leaves identical bit for bit: {identical}; {same.empty_leaves} empty "
          f"leaves; evaluation custom error {same.initial_error} -> {same.history[-1]}")

    rounds = dict(num_boost_round=model.n_trees, early_stopping_rounds=model.n_trees)
    model.refresh_device(*data)                      # warm
    trainer.fit_device(*data, **rounds)
    refresh_ms, fit_ms = [], []
    for _ in range(repetitions):                     # alternating, one process
        mark = time.perf_counter()
        model.refresh_device(*data).model.close()
        refresh_ms.append((time.perf_counter() - mark) * 1000.0)
        mark = time.perf_counter()
        trainer.fit_device(*data, **rounds).close()
        fit_ms.append((time.perf_counter() - mark) * 1000.0)
    print(f"{model.n_trees} trees over {sets.n_train} rows, median (min .. max) of {repetitions} warm calls:")
    for name, samples in (("refresh_device", refresh_ms), ("fit_device (cuts, bins, rounds)", fit_ms)):
        print(f"  {name:<34} {np.median(samples):9.2f} ms ({min(samples):.2f} .. {max(samples):.2f})")
    sets.free()
    trainer.close()

    new_titles, new_ids = titles_of(second)
    result = ds.refresh_model(truth_titles, first.title_id, new_titles, new_ids, model)
    changed = int(np.count_nonzero(result.model.arrays["threshold"] != model.arrays["threshold"]))
    leaves = int(np.count_nonzero(model.arrays["feature"] < 0))
    print(f"refreshed on a second draw of {len(new_titles)} train titles ({result.margins.shape[0]} rows): {changed} of "
          f"{leaves} leaves changed, {result.empty_leaves} without evidence; its evaluation custom error: the model as "
          f"given {result.initial_error}, refreshed {result.history[-1]} (best prefix {result.best_iteration + 1} trees: "
          f"{result.history[result.best_iteration]}); " + ", ".join(f"{k} {v:.1f} ms" for k, v in result.timings.items()))
    by_gain, by_count = result.gain_importance(), model.feature_importance()
    print("features by gain on the new rows (share of gain; share of splits):")
    for f in np.argsort(-by_gain, kind="stable")[:8]:
        print(f"  {ds.FEATURE_NAMES[f]:<24} {by_gain[f]:.3f}   {by_count[f]:.3f}")
    root = result.cover[model.arrays["tree_offsets"][:-1]]
    print(f"cover of the roots (hessian sums): {root.min():.1f} .. {root.max():.1f}")
    return same, result, refresh_ms, fit_ms


def _option(arguments, name, default, convert):
    if name not in arguments:
        return default
    at = arguments.index(name)
    if at + 1 >= len(arguments):
        raise SystemExit(f"{name} needs a value")
    value = convert(arguments[at + 1])
    del arguments[at:at + 2]
    return value


if __name__ == "__main__":
    arguments = sys.argv[1:]
    path = _option(arguments, "--model", None, str)
    repetitions = _option(arguments, "--timed", 5, int)
    main(*[int(a) for a in arguments[:2]], model_path=path, repetitions=repetitions)
