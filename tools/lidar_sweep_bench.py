#!/usr/bin/env python3
"""Time of one lidar callback: the raw sweep through set_lidar_sweep against what a robot pays today AFTER its host
node, set_scan_source fed the already segmented cloud.

  python tools/lidar_sweep_bench.py --parent-lib libdddmr_rollout_parent.so --out profiles/r14_lidar_sweep.json

parent side (a library built from the parent commit: `make OUT=libdddmr_rollout_parent.so` there, copied beside the new
one; selected through DDDMR_LIB_NAME): set_scan_source on the cloud the node publishes on segmented_cloud_pure, produced
here by the NumPy restatement (tests/helpers/lidar_sweep_ref.py), 16-byte records.  The node's own time (projection,
ground removal, BFS on the host) is NOT in this figure and was not measured: the reference cannot be built here.  new
side: set_lidar_sweep on the raw sweep, which does the node's work and the scan feed.  Shapes: 16 x 1000 and 16 x 440
(the shipped ones) and 64 x 2048, the sweeps of tests/helpers/lidar_sweep_cases.py.

Every measurement runs in a child process of its own (`--worker`), the two libraries alternate --rounds times on one box;
a round's figure is the median of --passes timed calls after --warmup untimed ones, host clock around the call (it ends
in its own wait for the device).  A side's figure is the median of its rounds' medians, its spread their range.  No bar
is set: both figures and the difference are reported.  For the kernels' own time:
  rocprofv3 --kernel-trace --stats -- python tools/lidar_sweep_bench.py --worker new --shape 16x1000 --passes 50
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import numpy as np  # noqa: E402

SHAPES = {"16x1000": "16x1000-g7-m0.0", "16x440": "16x440-g7-m0.0", "64x2048": "64x2048-g7-m0.2"}
TBS = (0.1, 0.0, 0.6, 0.0, 0.0, 0.0, 1.0)
TGB = (1.0, -0.5, 0.0, 0.0, 0.0, 0.14943813, 0.98877108)
WINDOW, HEIGHT = 8.0, 1.8


def worker(args):
    import lidar_sweep_cases as Cs
    from dddmr_navigation_amd import configs
    from dddmr_navigation_amd.local_planner import LocalPlanner
    c, raw, ref = Cs.case(SHAPES[args.shape])
    segmented = np.ascontiguousarray(ref["cloud"])
    times, counts = [], None
    with LocalPlanner([configs.bench_theory("C2")], max_points=200_000) as lp:
        if args.worker == "new":
            a, kw = c.planner_args()
            lp.set_lidar_sweep_source(0, *a, max_sweep_points=len(raw), **kw)
        for i in range(args.warmup + args.passes):
            t0 = time.perf_counter()
            if args.worker == "new":
                counts = lp.set_lidar_sweep(0, raw, TBS, TGB, WINDOW, HEIGHT)
            else:
                counts = lp.set_scan_source(0, segmented, TBS, TGB, WINDOW, HEIGHT)
            t1 = time.perf_counter()
            if i >= args.warmup:
                times.append(t1 - t0)
    us = sorted(1e6 * t for t in times)
    out = {"worker": args.worker, "shape": args.shape, "raw_points": len(raw), "segmented_points": len(segmented), "counts": list(counts),
           "passes": len(us), "median_us": statistics.median(us), "p10_us": us[len(us) // 10], "p90_us": us[(9 * len(us)) // 10]}
    print("RESULT " + json.dumps(out), flush=True)


def run_worker(which, shape, lib, args):
    env = dict(os.environ)
    if lib:
        env["DDDMR_LIB_NAME"] = lib
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", which, "--shape", shape, "--passes", str(args.passes), "--warmup", str(args.warmup)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.worker_timeout)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"worker {which} / {shape} ended with {p.returncode}")       # nothing more is started on the GPU
    line = next(l for l in p.stdout.splitlines() if l.startswith("RESULT "))
    return json.loads(line[7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", choices=["parent", "new"])
    ap.add_argument("--shape", choices=sorted(SHAPES), default="16x1000")
    ap.add_argument("--parent-lib", help="file name of the parent commit's library beside the new one")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--passes", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--worker-timeout", type=int, default=120)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    if not args.parent_lib:
        ap.error("--parent-lib is required")
    report = {"protocol": "host clock around one call, median of %d calls per round, %d alternations of the parent's and the new library "
                          "in child processes on one box; spread = range of the rounds' medians.  parent = set_scan_source on the already "
                          "segmented cloud (the host node's own time is not included and was not measured); new = set_lidar_sweep on the "
                          "raw sweep" % (args.passes, args.rounds),
              "shapes": {}}
    for shape in ("16x1000", "16x440", "64x2048"):
        rounds = {"parent": [], "new": []}
        for r in range(args.rounds):
            rounds["parent"].append(run_worker("parent", shape, args.parent_lib, args))
            rounds["new"].append(run_worker("new", shape, None, args))
            print(shape, r, "parent %.1f us" % rounds["parent"][-1]["median_us"], "new %.1f us" % rounds["new"][-1]["median_us"], flush=True)
        fig = {}
        for k, rs in rounds.items():
            med = [x["median_us"] for x in rs]
            fig[k] = {"median_us": statistics.median(med), "spread_us": max(med) - min(med), "rounds": rs}
        fig["new_minus_parent_us"] = fig["new"]["median_us"] - fig["parent"]["median_us"]
        report["shapes"][shape] = fig
        print(shape, "parent %.1f +- %.1f us, new %.1f +- %.1f us, difference %.1f us" % (
            fig["parent"]["median_us"], fig["parent"]["spread_us"], fig["new"]["median_us"], fig["new"]["spread_us"], fig["new_minus_parent_us"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
