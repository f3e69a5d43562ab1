#!/usr/bin/env python3
"""Is model B better than model A?  Two saved models (ForestModel.save, such as examples/train_model.py writes) on the
evaluation rows of a training set built from raw titles, under one paired bootstrap on the GPU:

    truth titles + train titles with their ids (synthetic, the titles of examples/train_model.py)
             -> FeatureEngineering.generate_train_and_evaluation_data_sets (the evaluation rows and, per row, the
                train title whose candidates it was sampled for)
             -> ds.compare_models([a, b], evaluation, target, groups=the rows' train titles)

    python examples/compare_models.py a.npz b.npz [n_truth] [n_queries] [n_boot]

It prints each model's evaluation error fn + 5 * fp with its 95% interval, and the difference a - b replicate by
replicate: its interval and the share of replicates in which a has the smaller error.  An interval of the difference
that holds 0 says that another evaluation sample of the same size could have ordered the two models the other way.
The rows are resampled by train title (ten candidate rows each), not one by one: the rows of a title stand or fall
together.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import doppel_speller_amd as ds  # noqa: E402
from doppel_speller_amd import synth  # noqa: E402
from doppel_speller_amd.tuning import row_groups  # noqa: E402


def main(path_a, path_b, n_truth=20000, n_queries=4000, n_boot=2000):
    models = [ds.ForestModel.load(path_a), ds.ForestModel.load(path_b)]
    train = synth.make_workload(n_truth, n_queries, seed=11, query_seed=101)
    truth_titles = synth._to_strings(train.t_flat, train.t_off)
    train_titles = synth._to_strings(train.q_flat, train.q_off)
    train_ids = np.where(train.actual_row >= 0, train.title_id[np.maximum(train.actual_row, 0)], -1)
    fe = ds.FeatureEngineering(truth_titles, train.title_id, train_titles, train_ids)
    _, _, evaluation, target = fe.generate_train_and_evaluation_data_sets()
    groups = row_groups(fe.rows)[fe.rows["evaluation"].to_numpy()]
    result = ds.compare_models(models, evaluation, target, groups=groups, n_boot=n_boot, names=("a", "b"))
    print(f"{evaluation.shape[0]} evaluation rows in {result.n_units} groups, {result.n_boot} replicates")
    print(result.frame().to_string(index=False))
    d = result.difference("a", "b")
    print(f"a - b: {d.baseline:+g} on the rows as they are; over the replicates mean {d.mean:+.1f}, 95% interval "
          f"[{d.interval[0]:+.1f}, {d.interval[1]:+.1f}], a better in {d.share_better:.3f} of them")
    return result


if __name__ == "__main__":
    if len(sys.argv) < 3:
        raise SystemExit(__doc__)
    main(sys.argv[1], sys.argv[2], *[int(a) for a in sys.argv[3:6]])
