"""The truth index built on the host (ds_index_create) and on the device (ds_index_create_device), in one process, on
the truth side of the synthetic workload: a warm-up of each build, then the two alternated, the wall clock of the whole
create call (the device's includes the upload of the CSR), median and range; the two images are compared at every size.

    python scripts/index_build_timings.py [--sizes 500000 5000000] [--calls 3] [--host-threads 16] [--out FILE]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/index_build_timings.py --sizes N --device-only

The host build runs on --host-threads threads (DS_HOST_THREADS; default 16, the CPUs a job may use on the shared GPU
machines -- left alone it sizes itself by the whole machine, up to 32).  --device-only builds on the device once per
size after a warm-up and nothing else: the form to run under a kernel trace.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import doppel_speller_amd as ds  # noqa: E402
from doppel_speller_amd import synth  # noqa: E402
from doppel_speller_amd.match_maker import IMAGE_ARRAYS, IMAGE_SCALARS, NativeProblem  # noqa: E402


def truth_arrays(n_truth, seed):
    _, t_flat, t_off = synth.make_truth(n_truth, seed)
    problem = NativeProblem.from_flat(t_flat, t_off, np.zeros(1, np.uint8), np.zeros(1, np.int64), 3)
    arrays = problem.arrays()
    problem.close()
    return arrays["rowptr"], arrays["truth_idx"], arrays["idf32"], arrays["sums32"]


def timed_build(arrays, build):
    started = time.perf_counter()
    index = ds.TruthIndex(*arrays, build=build)     # the create call ends synchronised
    return index, (time.perf_counter() - started) * 1000.0


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--sizes", type=int, nargs="+", default=[500_000, 5_000_000])
    parser.add_argument("--calls", type=int, default=3, help="timed builds of each kind, alternated")
    parser.add_argument("--host-threads", type=int, default=16)
    parser.add_argument("--device-only", action="store_true")
    parser.add_argument("--seed", type=int, default=20260101)
    parser.add_argument("--out", default=None, help="JSON file for the per-call timings")
    args = parser.parse_args()
    os.environ["DS_HOST_THREADS"] = str(args.host_threads)

    report = []
    for n_truth in args.sizes:
        started = time.perf_counter()
        arrays = truth_arrays(n_truth, args.seed)
        print(f"{n_truth} rows, {arrays[0].shape[0] - 1} columns, {arrays[1].shape[0]} postings "
              f"(generated in {time.perf_counter() - started:.1f} s)", flush=True)
        if args.device_only:
            for call in range(2):
                index, ms = timed_build(arrays, "device")
                index.close()
                print(f"  device build {'warm-up' if call == 0 else 'traced'}: {ms:.1f} ms", flush=True)
            continue
        times = {"host": [], "device": []}
        for call in range(args.calls + 1):          # call 0 of each build warms it up and is where the images are compared
            indexes = {}
            for build in ("host", "device"):
                indexes[build], ms = timed_build(arrays, build)
                if call:
                    times[build].append(ms)
            if call == 0:
                host, device = indexes["host"].image(), indexes["device"].image()
                assert indexes["host"].info() == indexes["device"].info()
                for name in IMAGE_SCALARS + tuple(IMAGE_ARRAYS):
                    same = host[name] == device[name] if name in IMAGE_SCALARS else \
                        host[name].dtype == device[name].dtype and host[name].shape == device[name].shape and \
                        np.array_equal(host[name].reshape(-1).view(np.uint8), device[name].reshape(-1).view(np.uint8))
                    assert same, f"{n_truth} rows: '{name}' of the device build differs from the host's"
                print("  images equal: every array and scalar, byte for byte", flush=True)
                del host, device
            for index in indexes.values():
                index.close()
        line = {"rows": n_truth, "postings": int(arrays[1].shape[0]), "host_threads": args.host_threads}
        for build, values in times.items():
            line[build] = {"median_ms": round(float(np.median(values)), 1),
                           "range_ms": [round(min(values), 1), round(max(values), 1)], "calls": [round(v, 1) for v in values]}
        line["host_over_device"] = round(line["host"]["median_ms"] / line["device"]["median_ms"], 2)
        print(f"  host build (DS_HOST_THREADS={args.host_threads}): median {line['host']['median_ms']} ms, range "
              f"{line['host']['range_ms']}; device build (with the upload of the CSR): median "
              f"{line['device']['median_ms']} ms, range {line['device']['range_ms']}; host / device "
              f"{line['host_over_device']}", flush=True)
        report.append(line)
    if args.out and report:
        with open(args.out, "w") as handle:
            json.dump(report, handle, indent=1)


if __name__ == "__main__":
    main()
