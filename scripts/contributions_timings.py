"""Milliseconds of ds_forest_predict_device, ds_forest_cover_device and ds_forest_contributions_device (exact and
approximate) on the same rows: by default 100,000 rows x 66 features under a 300-tree, depth-5 model, one warm-up call
and one timed call each (HIP events on the null stream).  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--rows", type=int, default=100000)
    parser.add_argument("--trees", type=int, default=300)
    parser.add_argument("--depth", type=int, default=5)
    args = parser.parse_args()
    import doppel_speller_amd as ds
    from doppel_speller_amd import _lib, synth
    forest = synth.make_forest(n_trees=args.trees, depth=args.depth)
    model = ds.ForestModel(forest["feature"], forest["threshold"], forest["yes"], forest["no"], forest["missing"],
                           forest["tree_offsets"], forest["n_features"], forest["base_margin"])
    rng = np.random.RandomState(1)
    rows = rng.uniform(0, 100, (args.rows, 66)).astype(np.float32)
    rows[rng.rand(args.rows, 66) < 0.1] = np.nan
    d_rows = _lib.DeviceArray.from_host(rows)
    d_margins = _lib.DeviceArray((args.rows,), np.float32)
    d_out = _lib.DeviceArray((args.rows, 67), np.float64)
    timer = _lib.Timer()

    def timed(call):
        call()                                   # warm-up
        timer.start()
        call()
        timer.stop()
        _lib.check(_lib.lib().ds_stream_sync(_lib.pointer(None), 0), "sync")
        return round(timer.elapsed_ms(), 3)

    result = {"rows": args.rows, "trees": args.trees, "depth": args.depth}
    result["predict_ms"] = timed(lambda: model.predict_device(d_rows, args.rows, d_margins, None))
    result["cover_ms"] = timed(lambda: _lib.check(_lib.lib().ds_forest_cover_device(
        model.handle, d_rows.ptr, args.rows, _lib.pointer(None)), "ds_forest_cover_device"))
    model.set_cover(model.read_cover() + 32.0)   # every node positive
    result["contributions_ms"] = timed(lambda: model.predict_contributions_device(d_rows, args.rows, d_out))
    result["approximate_ms"] = timed(lambda: model.predict_contributions_device(d_rows, args.rows, d_out, True))
    total = d_out.to_host(64).sum(axis=1)
    result["finite"] = bool(np.isfinite(total).all())
    print(json.dumps(result))


if __name__ == "__main__":
    main()
