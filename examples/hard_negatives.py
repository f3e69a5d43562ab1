#!/usr/bin/env python3
"""The hard-negative loop on synthetic titles, on the GPU:

    train_model (the base set: 10 random candidates of every train title's top 100)
        -> FeatureEngineering.generate_device_hard_negatives (every candidate of every train title scored by that
           model on the device; per title the hard_n wrong ones it likes best, the base set's own pairs left out)
        -> ForestTrainer.fit_device(..., init_model=model) on base rows + mined rows, the matrix never leaving HBM

It prints the evaluation error matrix (at probability 0.9, the reference's decision rule) of the first model and of the
continued one, on the same evaluation rows.  Nothing is claimed about how the two compare: that has not been measured
here, and synthetic titles would not settle it.

    python examples/hard_negatives.py [--false-positives] [--mined-weight W] [n_truth] [n_queries] [hard_n] [more_rounds]

--false-positives mines only candidates whose margin is above log(9), the margin of probability 0.9: the false positives
of the decision rule.
--mined-weight W continues with the mined rows at sample weight W and the base rows at 1 (ForestTrainer's
sample_weight; the default, 1, is the unweighted call).
"""
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import doppel_speller_amd as ds  # noqa: E402
from doppel_speller_amd import synth  # noqa: E402


def main(n_truth=20000, n_queries=4000, hard_n=5, more_rounds=50, false_positives=False, mined_weight=None):
    w = synth.make_workload(n_truth, n_queries, seed=11, query_seed=101)
    truth_titles = synth._to_strings(w.t_flat, w.t_off)
    train_titles = synth._to_strings(w.q_flat, w.q_off)
    train_ids = np.where(w.actual_row >= 0, w.title_id[np.maximum(w.actual_row, 0)], -1)

    first = ds.train_model(truth_titles, w.title_id, train_titles, train_ids)
    model = first.model
    print(f"train_model: {first.rows.shape[0]} rows, {model.n_trees} trees; evaluation rows: TP {first.error_matrix[0]}  "
          f"TN {first.error_matrix[1]}  FP {first.error_matrix[2]}  FN {first.error_matrix[3]}")

    # the same base set, its matrices kept in HBM (the same seed gives the same rows and the same split)
    fe = ds.FeatureEngineering(truth_titles, w.title_id, train_titles, train_ids)
    sets = fe.generate_device_data_sets()
    assert fe.rows.equals(first.rows)
    before = ds.evaluation_error_matrix(model, sets.evaluation.to_host(sets.n_evaluation), sets.evaluation_target)

    hard = fe.generate_device_hard_negatives(model, hard_n=hard_n, min_margin=math.log(9) if false_positives else None)
    mined = fe.hard_rows
    print(f"mined {hard.n} hard negatives of {mined['query_index'].nunique()} train titles"
          + (f": margin {mined['margin'].min():.3f} .. {mined['margin'].max():.3f}, "
             f"{int((mined['probability'] > 0.9).sum())} above probability 0.9, median position "
             f"{int(mined['position'].median())} of {fe.top_n}" if hard.n else "")
          + "; " + ", ".join(f"{k} {v:.1f} ms" for k, v in fe.hard_timings.items()))

    joined = sets.with_hard_negatives(hard)
    weighted = {} if mined_weight is None else dict(
        sample_weight=np.concatenate((np.ones(sets.n_train), np.full(hard.n, mined_weight))))
    t0 = time.perf_counter()
    trainer = ds.ForestTrainer()
    continued = trainer.fit_device(joined.train, joined.n_train, joined.train_target, joined.evaluation,
                                   joined.n_evaluation, joined.evaluation_target, init_model=model,
                                   num_boost_round=more_rounds, **weighted)
    print(f"continued on {joined.n_train} rows ({sets.n_train} base + {hard.n} mined"
          + (f" at weight {mined_weight:g}" if mined_weight is not None else "") + f") for {len(trainer.history)} rounds "
          f"in {time.perf_counter() - t0:.2f}s: {continued.n_trees} trees (init model's custom error "
          f"{trainer.initial_error}, best new round's {min(trainer.history)})")
    after = ds.evaluation_error_matrix(continued, sets.evaluation.to_host(sets.n_evaluation), sets.evaluation_target)
    for name, (tp, tn, fp, fn) in (("before", before), ("after", after)):
        print(f"evaluation rows {name}: TP {tp}  TN {tn}  FP {fp}  FN {fn}")
    for owner in (hard, joined, sets):
        owner.free()
    return before, after


if __name__ == "__main__":
    arguments = [a for a in sys.argv[1:] if a != "--false-positives"]
    weight = None
    if "--mined-weight" in arguments:
        at = arguments.index("--mined-weight")
        if at + 1 >= len(arguments):
            raise SystemExit("--mined-weight needs a number, the sample weight of every mined row")
        weight = float(arguments[at + 1])
        del arguments[at:at + 2]
    main(*[int(a) for a in arguments[:4]], false_positives="--false-positives" in sys.argv[1:], mined_weight=weight)
