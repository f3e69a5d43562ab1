#!/usr/bin/env python3
"""What seeding a trainer from a model costs ("Continuing from a model", Measurements), on the
matrix of section 9's table: ROWS x 66 features, an evaluation set of ROWS / 10, depth 5.

    round    ForestTrainer.step(): the median of 10 rounds after 2 (the figure of section 9's table)
    predict  ForestModel.predict_device of a TREES-tree model over both matrices in HBM (margins only), then a sync
    seed     ds_trainer_seed_device of the same model over the same two matrices (the call ends in its own sync)

predict and seed: the median of 10 calls after 2 warm-up calls, alternated; every seed call takes a fresh trainer (a
trainer is seeded once), created outside the timed window.

    python scripts/continue_timings.py [rows] [trees] [--round-only]

--round-only stops after the round's figure (for a library without the seed entry points, named by DS_LIBRARY).
"""
import ctypes
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import doppel_speller_amd as ds  # noqa: E402
from doppel_speller_amd import _lib  # noqa: E402


def data(n, nf=66, seed=3):
    rng = np.random.RandomState(seed)
    x = rng.randn(n, nf).astype(np.float32)
    y = (x[:, 0] + 0.5 * x[:, 1] * x[:, 2] + 0.5 * rng.randn(n) > 1.0).astype(np.float32)
    return x, y


def report(name, times, note=""):
    print(f"{name:8s} median {statistics.median(times):.3f} ms ({min(times):.3f}-{max(times):.3f}, {len(times)} runs){note}",
          flush=True)


def main(n=1000000, trees=300, round_only=False):
    x, y = data(n)
    n_eval = n // 10
    ex, ey = x[:n_eval], y[:n_eval]
    trainer = ds.ForestTrainer().begin(x, y, ex, ey)
    times = []
    for _ in range(12):
        mark = time.perf_counter()
        trainer.step()
        times.append((time.perf_counter() - mark) * 1000.0)
    report("round", times[2:], f"  n={n}, depth 5")
    if round_only:
        trainer.close()
        return
    for _ in range(trees - 12):
        trainer.step()
    model = trainer.model()
    trainer.close()
    nodes = model.n_nodes
    d_x, d_ex = _lib.DeviceArray.from_host(x), _lib.DeviceArray.from_host(ex)
    d_margins, d_eval_margins = _lib.DeviceArray((n,), np.float32), _lib.DeviceArray((n_eval,), np.float32)
    library = _lib.lib()
    predict, seed = [], []
    for _ in range(12):
        mark = time.perf_counter()
        model.predict_device(d_x, n, d_margins)
        model.predict_device(d_ex, n_eval, d_eval_margins)
        _lib.check(library.ds_stream_sync(None, 0), "ds_stream_sync")
        predict.append((time.perf_counter() - mark) * 1000.0)
        fresh = ds.ForestTrainer().begin_device(d_x, n, y, d_ex, n_eval, ey)
        error = ctypes.c_int64(-1)
        mark = time.perf_counter()
        _lib.check(library.ds_trainer_seed_device(fresh.handle, model.handle, d_x.ptr, d_ex.ptr, ctypes.byref(error),
                                                  None), "ds_trainer_seed_device")
        seed.append((time.perf_counter() - mark) * 1000.0)
        same = fresh.margins().tobytes() == d_margins.to_host().tobytes() and \
            fresh.eval_margins().tobytes() == d_eval_margins.to_host().tobytes()
        fresh.close()
        if not same:
            raise SystemExit("the seeded margins differ from predict_device's")
    note = f"  {model.n_trees} trees, {nodes} nodes, {n} + {n_eval} rows"
    report("predict", predict[2:], note)
    report("seed", seed[2:], note + f", initial error {error.value}")
    for array in (d_x, d_ex, d_margins, d_eval_margins):
        array.free()


if __name__ == "__main__":
    arguments = [a for a in sys.argv[1:] if not a.startswith("--")]
    main(*(int(a) for a in arguments[:2]), round_only="--round-only" in sys.argv)
