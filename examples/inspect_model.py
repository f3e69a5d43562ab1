#!/usr/bin/env python3
"""Which features a match model needs and how its margin moves along one of them, on the GPU and on synthetic data:

    the training and evaluation sets of examples/train_model.py (FeatureEngineering on synthetic titles)
             -> ForestTrainer.fit, or --model model.npz (a ForestModel saved by examples/train_model.py)
             -> ForestModel.permutation_importance on the evaluation set: 66 features x --repeats shuffles + the
                baseline, one launch (csrc/ds_inspect.hip)
             -> ForestModel.partial_dependence of title_ratio

It prints the ten most important features next to their rank by split count (ForestModel.feature_importance, the
reference's get_fscore), the partial dependence, and the time of the device call (warm, --timed repetitions: the
host-array form, which uploads the matrix once, and the form for a matrix already in HBM) next to the same counts made
the only way there was before: a host loop of 66 x repeats + 1 calls of ForestModel.predict on host-shuffled copies,
each of which uploads the whole matrix.

    python examples/inspect_model.py [--model model.npz] [--repeats 5] [--timed 5] [n_truth] [n_queries]
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import doppel_speller_amd as ds  # noqa: E402
from doppel_speller_amd import _lib, synth  # noqa: E402
from doppel_speller_amd.train import _error_matrix  # noqa: E402


def host_loop(model, rows, target, n_repeats, beta=5.0, seed=0):
    """Permutation importance without the inspection kernel: every shuffled copy goes through ForestModel.predict."""
    rng = np.random.RandomState(seed)
    tp, tn, fp, fn = _error_matrix(model.predict(rows), target, 0.9)
    baseline = fn + beta * fp
    importance = np.zeros(rows.shape[1])
    for f in range(rows.shape[1]):
        errors = []
        for _ in range(n_repeats):
            shuffled = rows.copy()
            shuffled[:, f] = rows[rng.permutation(rows.shape[0]), f]
            tp, tn, fp, fn = _error_matrix(model.predict(shuffled), target, 0.9)
            errors.append(fn + beta * fp)
        importance[f] = np.mean(errors) - baseline
    return importance


def timed(call, repetitions):
    """Milliseconds of `repetitions` warm calls, each ending in a device synchronisation: (median, min, max)."""
    call()
    samples = []
    for _ in range(repetitions):
        mark = time.perf_counter()
        call()
        samples.append((time.perf_counter() - mark) * 1000.0)
    return float(np.median(samples)), min(samples), max(samples)


def main(n_truth=20000, n_queries=4000, model_path=None, n_repeats=5, repetitions=5):
    train = synth.make_workload(n_truth, n_queries, seed=11, query_seed=101)
    truth_titles = synth._to_strings(train.t_flat, train.t_off)
    train_titles = synth._to_strings(train.q_flat, train.q_off)
    train_ids = np.where(train.actual_row >= 0, train.title_id[np.maximum(train.actual_row, 0)], -1)
    fe = ds.FeatureEngineering(truth_titles, train.title_id, train_titles, train_ids)
    features, labels, eval_features, eval_labels = fe.generate_train_and_evaluation_data_sets()
    if model_path:
        model = ds.ForestModel.load(model_path)
    else:
        model = ds.ForestTrainer().fit(features, labels, eval_features, eval_labels)
    n = eval_features.shape[0]
    print(f"model: {model.n_trees} trees, {model.n_nodes} nodes; evaluation set: {n} rows, {int(eval_labels.sum())} positive")

    importance = model.permutation_importance(eval_features, eval_labels, n_repeats=n_repeats)
    tp, tn, fp, fn = importance.baseline
    print(f"baseline: TP {tp}  TN {tn}  FP {fp}  FN {fn}, custom error {importance.baseline_error:g}")
    shares = model.feature_importance()
    split_rank = {int(f): rank for rank, f in enumerate(np.argsort(-shares, kind="stable"), 1)}
    print(f"permutation importance, {n_repeats} shuffles per feature (error increase; rank by split count):")
    for _, row in importance.frame().head(10).iterrows():
        print(f"  {row['name']:<24} +{row['importance']:8.1f} (std {row['importance_std']:6.1f})   mean margin "
              f"{row['margin_shift']:+.4f}   split-count rank {split_rank[int(row['feature'])]:2d} "
              f"({shares[int(row['feature'])]:.3f})")
    unused = int(np.count_nonzero((importance.importance == 0) & (importance.importance_std == 0)))
    print(f"  {unused} of {ds.FEATURES_COUNT} features leave the error as it is in every shuffle")

    dependence = model.partial_dependence(eval_features, "title_ratio", n_grid=12)
    print(f"partial dependence of title_ratio (mean margin of the {n} rows; unchanged: "
          f"{dependence.baseline_mean_margin:+.4f}):")
    for value, margin, share in zip(dependence.grid, dependence.mean_margin, dependence.positive_share):
        print(f"  title_ratio = {value:8.3f}   mean margin {margin:+.4f}   above 0.9: {share:.4f}")

    jobs = 1 + ds.FEATURES_COUNT * n_repeats
    d_rows = _lib.DeviceArray.from_host(eval_features)
    d_target = _lib.DeviceArray.from_host(np.ascontiguousarray(eval_labels, dtype=np.float32))
    host_form = timed(lambda: model.permutation_importance(eval_features, eval_labels, n_repeats=n_repeats), repetitions)
    hbm_form = timed(lambda: model.permutation_importance_device(d_rows, n, d_target, n_repeats=n_repeats), repetitions)
    loop = timed(lambda: host_loop(model, eval_features, eval_labels, n_repeats), max(3, repetitions // 2))
    d_rows.free()
    d_target.free()
    print(f"{jobs} jobs over {n} rows x {model.n_trees} trees, median (min .. max) of warm calls:")
    print(f"  permutation_importance (host matrix, one launch)        {host_form[0]:9.2f} ms ({host_form[1]:.2f} .. {host_form[2]:.2f})")
    print(f"  permutation_importance_device (matrix in HBM)           {hbm_form[0]:9.2f} ms ({hbm_form[1]:.2f} .. {hbm_form[2]:.2f})")
    print(f"  host loop of {jobs} ForestModel.predict calls             {loop[0]:9.2f} ms ({loop[1]:.2f} .. {loop[2]:.2f})")
    return importance, dependence, host_form, hbm_form, loop


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
    repeats = _option(arguments, "--repeats", 5, int)
    repetitions = _option(arguments, "--timed", 5, int)
    main(*[int(a) for a in arguments[:2]], model_path=path, n_repeats=repeats, repetitions=repetitions)
