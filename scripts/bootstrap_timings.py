"""The paired bootstrap at the size of examples/train_model.py ("Is a difference real"): two models
trained on its synthetic titles, one unconstrained and one under ratio_constraints(), compared on the evaluation rows
grouped by train title with B replicates.  Times, each the median [min, max] of --repeats calls after one warm-up, by
the host clock around a call that ends with the counts on the host:

    compare_models_device   the evaluation matrix and its target already in HBM
    compare_models          the same call from the host matrix (uploads it first)
    the oracle              tests/bootstrap_oracle.py doing the same counts with NumPy, from predict's margins

and what the tool says about the two models.  The three give the same counts (checked).  Which form of the kernel a
run takes is printed with it: a unit table is 16 bytes per group and model and is staged in LDS up to 128 KiB, so the
6,018 groups x 2 models of this size read it from HBM / L2.  Last, the two forms against each other where both apply:
ds.bootstrap_counts on the rows of the first --lds-groups groups, "table_in_lds" 0 and 1 alternated in one process.

    python scripts/bootstrap_timings.py [--truth 20000] [--train 4000] [--boot 2000] [--repeats 5]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bootstrap_oracle as oracle  # noqa: E402
import doppel_speller_amd as ds  # noqa: E402
from doppel_speller_amd import _lib, synth  # noqa: E402
from doppel_speller_amd.tuning import row_groups  # noqa: E402


def timed(call, repeats):
    call()
    ms = []
    for _ in range(repeats):
        mark = time.perf_counter()
        out = call()
        ms.append((time.perf_counter() - mark) * 1000.0)
    return out, f"{np.median(ms):.2f} ms [{min(ms):.2f}, {max(ms):.2f}]"


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--truth", type=int, default=20000)
    parser.add_argument("--train", type=int, default=4000)
    parser.add_argument("--boot", type=int, default=2000)
    parser.add_argument("--repeats", type=int, default=5)
    parser.add_argument("--lds-groups", type=int, nargs="*", default=[2000, 4000])
    args = parser.parse_args()
    w = synth.make_workload(args.truth, args.train, seed=11, query_seed=101)
    truth, train = synth._to_strings(w.t_flat, w.t_off), synth._to_strings(w.q_flat, w.q_off)
    ids = np.where(w.actual_row >= 0, w.title_id[np.maximum(w.actual_row, 0)], -1)
    plain = ds.train_model(truth, w.title_id, train, ids).model
    monotone = ds.train_model(truth, w.title_id, train, ids, monotone_constraints=ds.ratio_constraints()).model
    fe = ds.FeatureEngineering(truth, w.title_id, train, ids)
    _, _, evaluation, target = fe.generate_train_and_evaluation_data_sets()
    groups = row_groups(fe.rows)[fe.rows["evaluation"].to_numpy()]
    models, names = [monotone, plain], ("monotone", "unconstrained")
    n = evaluation.shape[0]
    d_rows = _lib.DeviceArray.from_host(evaluation)
    d_target = _lib.DeviceArray.from_host(np.ascontiguousarray(target, dtype=np.float32))
    keywords = dict(groups=groups, n_boot=args.boot, seed=0, names=names)
    device, device_ms = timed(lambda: ds.compare_models_device(models, d_rows, n, d_target, **keywords), args.repeats)
    host, host_ms = timed(lambda: ds.compare_models(models, evaluation, target, **keywords), args.repeats)
    unit, n_units = oracle.dense_units(groups)

    def restated():
        codes = np.stack([oracle.model_codes(model.predict(evaluation, output_margin=True), target, 0.9)
                          for model in models])
        return oracle.counts(codes, unit, n_units, args.boot, 0)
    (expected, baseline), oracle_ms = timed(restated, min(args.repeats, 3))
    assert device.counts.tobytes() == host.counts.tobytes() == expected.tobytes()
    assert device.baseline_counts.tobytes() == baseline.tobytes()
    rows_only, rows_ms = timed(lambda: ds.compare_models_device(models, d_rows, n, d_target, n_boot=args.boot, names=names),
                               args.repeats)

    def form(table_bytes):
        return "table staged in LDS" if table_bytes <= oracle.LDS_TABLE_BYTES else "table read from HBM / L2"
    grouped, by_row = form(16 * n_units * len(models)), form(n * ((len(models) + 3) // 4 * 4))
    print(f"{n} evaluation rows in {n_units} groups, {len(models)} models, {args.boot} replicates")
    print(f"compare_models_device (matrix in HBM)   {device_ms}   unit table of {16 * n_units * len(models)} B: {grouped}")
    print(f"compare_models (host matrix)            {host_ms}   {grouped}")
    print(f"tests/bootstrap_oracle.py (NumPy)       {oracle_ms}")
    print(f"compare_models_device, rows as units    {rows_ms}   codes of {n * 4} B: {by_row}")
    codes = np.stack([oracle.model_codes(model.predict(evaluation, output_margin=True), target, 0.9) for model in models])
    for wanted in args.lds_groups:
        keep = unit < wanted
        part, part_unit = np.ascontiguousarray(codes[:, keep]), unit[keep]
        ms = {0: [], 1: []}
        for call in range(2 * (args.repeats + 1)):
            in_lds = call % 2
            _lib.check(_lib.lib().ds_bootstrap_option(b"table_in_lds", in_lds), "ds_bootstrap_option")
            mark = time.perf_counter()
            got = ds.bootstrap_counts(part, part_unit, n_boot=args.boot)
            if call >= 2:
                ms[in_lds].append((time.perf_counter() - mark) * 1000.0)
            assert got.n_units == min(wanted, n_units)
        _lib.check(_lib.lib().ds_bootstrap_option(b"table_in_lds", 1), "ds_bootstrap_option")
        print(f"bootstrap_counts, {part.shape[1]} rows in {got.n_units} groups, table of {32 * got.n_units} B: from LDS "
              f"{np.median(ms[1]):.2f} ms [{min(ms[1]):.2f}, {max(ms[1]):.2f}], from HBM / L2 {np.median(ms[0]):.2f} ms "
              f"[{min(ms[0]):.2f}, {max(ms[0]):.2f}]")
    print(device.frame().to_string(index=False))
    for result, what in ((device, "by train title"), (rows_only, "by row")):
        d = result.difference("monotone", "unconstrained")
        print(f"monotone - unconstrained, resampled {what}: {d.baseline:+g}; mean {d.mean:+.2f}, standard error "
              f"{d.standard_error:.2f}, 95% interval [{d.interval[0]:+.1f}, {d.interval[1]:+.1f}], share_better "
              f"{d.share_better:.4f}")


if __name__ == "__main__":
    main()
