#!/usr/bin/env python3
"""Time of set_lidar_sweep with the sweep's features on, without and with the sweep association, against the parent
commit's set_lidar_sweep with features on, on the same sweeps (tools/lidar_features_bench.py's conventions and shapes).

  python tools/sweep_association_bench.py --parent-lib libdddmr_rollout_parent.so --out profiles/r32_sweep_association.json

parent: a library built from the parent commit (`make OUT=libdddmr_rollout_parent.so` there, copied beside the new one;
selected through DDDMR_LIB_NAME), features on.  features: the new library, features on, the association never switched
on -- the path is meant to launch what it launched, and the condition reported is |median(features) - median(parent)| <=
the parent's own p10-p90 spread in this run.  assoc: the new library after set_lidar_sweep_association; its increment
over `features` is reported as a median with the p10-p90 of the rounds' increments, and no bar is set on it: what it
replaces is the host node's second pass over the sweep, whose time is NOT in any figure here and was not measured.

Every measurement runs in a child process of its own (`--worker`), the three alternate --rounds times on one box; a
round's figure is the median of --passes timed calls after --warmup untimed ones, host clock around the call (it ends in
its own wait for the device).  A side's figure is the median of its rounds' medians; p10 / p90 are the medians of the
rounds' p10 / p90.
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

SHAPES = {"16x1000": "16x1000-g7-m0.0", "16x2000": "16x2000-floor-wall", "64x2048": "64x2048-g7-m0.2"}
TBS = (0.1, 0.0, 0.6, 0.0, 0.0, 0.0, 1.0)
TGB = (1.0, -0.5, 0.0, 0.0, 0.0, 0.14943813, 0.98877108)
WINDOW, HEIGHT = 8.0, 1.8
SIDES = ("parent", "features", "assoc")


def worker(args):
    import lidar_features_cases as FC
    import lidar_features_ref as FR
    from dddmr_navigation_amd import configs
    from dddmr_navigation_amd.local_planner import LocalPlanner
    c, raw, ref, feat = FC.case(SHAPES[args.shape])
    times, counts, n_assoc = [], None, None
    with LocalPlanner([configs.bench_theory("C2")], max_points=200_000) as lp:
        a, kw = c.planner_args()
        lp.set_lidar_sweep_source(0, *a, max_sweep_points=len(raw), **kw)
        lp.set_lidar_sweep_features(0, FC.EDGE, FC.SURF, T_out=FR.node_T())
        sa = None
        if args.worker == "assoc":
            from dddmr_navigation_amd.sweep_association import SweepAssociation
            sa = SweepAssociation(lp, 0, 0.1)
        for i in range(args.warmup + args.passes):
            t0 = time.perf_counter()
            counts = lp.set_lidar_sweep(0, raw, TBS, TGB, WINDOW, HEIGHT)
            t1 = time.perf_counter()
            if i >= args.warmup:
                times.append(t1 - t0)
        n_feat = [len(lp.get_lidar_sweep_features(0, w)[1]) for w in range(3)]
        assert n_feat == [len(l) for l in feat["lists"]], (n_feat, [len(l) for l in feat["lists"]])
        if sa is not None:
            n_assoc = {"less_flat": len(sa.cloud(3)[1]), "outliers": len(sa.outliers()), "half_index": sa.orientation()[3]}
            assert len(sa.times()) == len(feat["seg"]["range"])
    us = sorted(1e6 * t for t in times)
    out = {"worker": args.worker, "shape": args.shape, "raw_points": len(raw), "segmented_cloud_points": len(feat["seg"]["range"]),
           "counts": list(counts), "features": n_feat, "association": n_assoc, "passes": len(us), "median_us": statistics.median(us),
           "p10_us": us[len(us) // 10], "p90_us": us[(9 * len(us)) // 10]}
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
    ap.add_argument("--worker", choices=SIDES)
    ap.add_argument("--shape", choices=sorted(SHAPES), default="16x1000")
    ap.add_argument("--shapes", default="16x1000,16x2000,64x2048")
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
    report = {"protocol": "host clock around one set_lidar_sweep call, median of %d calls per round after %d untimed ones, %d alternations of "
                          "parent / features / assoc in child processes on one box; parent = the parent commit's library with features on, "
                          "features = this library with features on and the association never switched on, assoc = after "
                          "set_lidar_sweep_association.  The host node's own time is not included in any figure and was not measured"
                          % (args.passes, args.warmup, args.rounds),
              "shapes": {}}
    for shape in args.shapes.split(","):
        rounds = {k: [] for k in SIDES}
        for r in range(args.rounds):
            rounds["parent"].append(run_worker("parent", shape, args.parent_lib, args))
            rounds["features"].append(run_worker("features", shape, None, args))
            rounds["assoc"].append(run_worker("assoc", shape, None, args))
            print(shape, r, " ".join("%s %.1f us" % (k, rounds[k][-1]["median_us"]) for k in rounds), flush=True)
        fig = {}
        for k, rs in rounds.items():
            fig[k] = {key: statistics.median(x[key] for x in rs) for key in ("median_us", "p10_us", "p90_us")}
            fig[k]["rounds"] = rs
        spread = fig["parent"]["p90_us"] - fig["parent"]["p10_us"]
        fig["features_minus_parent_us"] = fig["features"]["median_us"] - fig["parent"]["median_us"]
        fig["parent_p10_p90_spread_us"] = spread
        fig["features_within_parent_spread"] = abs(fig["features_minus_parent_us"]) <= spread
        inc = sorted(a["median_us"] - f["median_us"] for a, f in zip(rounds["assoc"], rounds["features"]))
        fig["assoc_minus_features_us"] = {"median": statistics.median(inc), "p10": inc[len(inc) // 10], "p90": inc[(9 * len(inc)) // 10],
                                          "rounds": inc}
        report["shapes"][shape] = fig
        print(shape, "parent %.1f us (p10-p90 %.1f), features %+.1f us (within the spread: %s), association %+.1f us over features" % (
            fig["parent"]["median_us"], spread, fig["features_minus_parent_us"], fig["features_within_parent_spread"],
            fig["assoc_minus_features_us"]["median"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
