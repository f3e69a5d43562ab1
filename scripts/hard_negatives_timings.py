#!/usr/bin/env python3
"""The stages of FeatureEngineering.generate_device_hard_negatives ("Hard negatives", Measured):
`hard_timings` of one warm call per workload, so that `select` stands beside `features` and `model` of the same call.

    small   the workload of tests/test_gpu_hard_negatives.py: 300 truth titles, 60 train titles, top_n 20, sample_n 4,
            hard_n 3, a 12-tree forest
    large   N_TRUTH truth titles, N_TRAIN train titles, top_n 100, sample_n 10, hard_n 5, the random 100-tree stand-in
            forest of the other examples (synth.make_forest: trained trees are no costlier to walk)

    python scripts/hard_negatives_timings.py [n_truth] [n_train]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import doppel_speller_amd as ds  # noqa: E402
from doppel_speller_amd import synth  # noqa: E402
from doppel_speller_amd.training_set import row_plan  # noqa: E402


def run(name, n_truth, n_train, seed, model, top_n, sample_n, hard_n):
    w = synth.make_workload(n_truth, n_train, seed=seed, query_seed=seed + 1)
    truth, train = synth._to_strings(w.t_flat, w.t_off), synth._to_strings(w.q_flat, w.q_off)
    ids = np.where(w.actual_row >= 0, w.title_id[np.maximum(w.actual_row, 0)], -1)
    fe = ds.FeatureEngineering(truth, w.title_id, train, ids, top_n=top_n, sample_n=sample_n, transform=False)
    fe.generate_device_data_sets().free()
    for _ in range(2):                       # the second call is the warm one
        hard = fe.generate_device_hard_negatives(model, hard_n=hard_n)
        mined = hard.n
        hard.free()
    titles = sum(rows.shape[0] for rows in row_plan(fe.train_truth_rows))
    print(f"{name}: {n_truth} truth titles, {titles} selected train titles x top_n {top_n} = {titles * top_n} pairs scored, "
          f"{mined} mined (hard_n {hard_n}); " + ", ".join(f"{k} {v:.3f} ms" for k, v in fe.hard_timings.items()), flush=True)


def main(n_truth=20000, n_train=4000):
    from test_forest_cpu import random_dump
    run("small", 300, 60, 31, ds.ForestModel.from_xgboost_dump(random_dump(6, n_trees=12), ds.FEATURES_COUNT), 20, 4, 3)
    f = synth.make_forest(n_trees=100)
    stand_in = ds.ForestModel(f["feature"], f["threshold"], f["yes"], f["no"], f["missing"], f["tree_offsets"],
                              f["n_features"], f["base_margin"])
    run("large", n_truth, n_train, 11, stand_in, 100, 10, 5)


if __name__ == "__main__":
    main(*[int(a) for a in sys.argv[1:3]])
