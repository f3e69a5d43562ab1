#!/usr/bin/env python3
"""Learn how titles get misspelled from labelled pairs, on the GPU, and generate training rows that follow it:

    train titles with the id of their truth title
             -> ds.fit_misspelling_profile (every pair aligned on the device, one wave per pair; pairs further apart
                than max_edits are other names, not typos, and only counted as skipped)
             -> the report: edits per title, the share of each operation, how many letter substitutions are neighbours
                on the keyboard (the only ones the reference's generator makes), the most frequent confusions
             -> ten truth titles misspelled by the reference's generator and by the learned one, side by side

    python examples/learn_misspellings.py [--train] [--max-edits N] [n_truth] [n_queries]

--train also trains the match model twice with ds.train_model, without and with misspelling_profile="fit", and prints
both evaluation error matrices.  The synthetic train titles here were made by the reference's own rule (synth), so the
learned profile can only rediscover that rule: the comparison says nothing about real data.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import doppel_speller_amd as ds  # noqa: E402
from doppel_speller_amd import synth  # noqa: E402


def main(n_truth=20000, n_queries=4000, train=False, max_edits=4):
    w = synth.make_workload(n_truth, n_queries, seed=11, query_seed=101)
    truth_titles = synth._to_strings(w.t_flat, w.t_off)
    train_titles = synth._to_strings(w.q_flat, w.q_off)
    train_ids = np.where(w.actual_row >= 0, w.title_id[np.maximum(w.actual_row, 0)], -1)
    labelled = np.nonzero(w.actual_row >= 0)[0]
    pairs = ([truth_titles[w.actual_row[i]] for i in labelled], [train_titles[i] for i in labelled])

    profile = ds.fit_misspelling_profile(*pairs, max_edits=max_edits)
    print(f"{labelled.shape[0]} labelled pairs of {n_queries} train titles")
    print(profile.report())

    scripts = ds.edit_operations(pairs[0][:200], pairs[1][:200])
    for i in np.nonzero(scripts.distance > 0)[0][:3]:
        print(f"\npair {i}, {scripts.distance[i]} edits:\n" + scripts.render(i))

    sample = [t for t in ds.transform_titles(truth_titles) if len(t) > 9][:10]
    by_rule = ds.generate_misspelled_names(sample, seed=1)
    by_profile = ds.generate_misspelled_names(sample, seed=1, profile=profile)
    width = max(len(t) for t in sample + by_rule)
    print(f"\n{'title':<{width}}  {'reference generator':<{width}}  learned profile")
    for row in zip(sample, by_rule, by_profile):
        print(f"{row[0]:<{width}}  {row[1]:<{width}}  {row[2]}")

    if train:
        for name, argument in (("reference generator", None), ("learned profile", "fit")):
            result = ds.train_model(truth_titles, w.title_id, train_titles, train_ids, misspelling_profile=argument)
            tp, tn, fp, fn = result.error_matrix
            print(f"{name:<20} evaluation rows: TP {tp}  TN {tn}  FP {fp}  FN {fn}   custom error {fn + 5 * fp}, "
                  f"{result.model.n_trees} trees")
    return profile


if __name__ == "__main__":
    arguments = [a for a in sys.argv[1:] if a != "--train"]
    edits = 4
    if "--max-edits" in arguments:
        at = arguments.index("--max-edits")
        if at + 1 >= len(arguments):
            raise SystemExit("--max-edits needs a number in 0 .. 32")
        edits = int(arguments[at + 1])
        del arguments[at:at + 2]
    main(*[int(a) for a in arguments[:2]], train="--train" in sys.argv[1:], max_edits=edits)
