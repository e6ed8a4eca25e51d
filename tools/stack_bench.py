#!/usr/bin/env python3
"""Time of one perception pass of a robot with a lidar and two depth cameras, the stack against what a caller had to do
before it.

  python tools/stack_bench.py --parent-lib libdddmr_rollout_parent.so --out profiles/r13_stack.json

parent sequence (a library built from the parent commit: `make OUT=libdddmr_rollout_parent.so` there, copied beside the
new one; selected through DDDMR_LIB_NAME): marking_update + marking_get_dgraph + marking_get_lethal in one context,
depth_layer_update + depth_layer_get_dgraph + depth_layer_get_lethal in a second one (one context is wrong there: the
lidar layer would mark the cameras' points), then the minimum over the static layer and the two on the host (NumPy, reported
separately).  new sequence: stack_update + stack_get_changes in one context (the full getters when the list overflowed,
counted).  The scene is tests/helpers/stack_cases.py's, its five updates' feeds cycled; the feeds are not timed.  Two
grounds: the scene's own 4225 nodes, and the same lattice tiled 16 x 16 (1.08e6 nodes, the scene over the first tile).

Every measurement runs in a child process of its own (`--worker`), the two libraries alternate --rounds times on one box;
a round's figure is the median of --passes timed passes after --warmup untimed ones, host clock around the pass (every
call in it ends in its own wait for the device).  A sequence's figure is the median of its rounds' medians, its spread
their range.  The bars: at the large ground new < parent - parent's spread; at the small one new <= parent + parent's
spread.  For the kernel's own time:
  rocprofv3 --kernel-trace --stats -- python tools/stack_bench.py --worker new --ground large --passes 50
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

TILES = 16


def scene(ground_kind):
    import depth_layer_cases as cases
    import stack_cases as sc
    case = sc.SEQUENCE
    ups = cases.updates(case)
    ups = [dict(u, feeds=[sc.lidar_feed(k, u["t_gb"])] + [f for f in u["feeds"] if f["kind"] != "lidar"]) for k, u in enumerate(ups)]
    ground = cases.ground_of(case)
    if ground_kind == "large":
        pitch = 65 * 0.25
        tiles = [ground + np.array([i * pitch, j * pitch, 0.0], np.float32) for i in range(TILES) for j in range(TILES)]
        ground = np.concatenate(tiles, axis=0).astype(np.float32)        # tile (0, 0) first: node numbers of the scene's own ground stay
    static = np.full(len(ground) + 1, 9999.0)
    static[: 4225] = sc.static_layer(ground[:4225])[:4225]
    return case, ups, ground, static, sc


def feed(lp, st):
    import depth_clear_cases as dc
    if st["kind"] == "lidar":
        lp.set_scan_source(st["sid"], st["data"], st["t_bs"], st["t_gb"], 5.0, 2.0)
    else:
        lp.set_depth_frame(st["sid"], st["data"], st["t_bs"], st["t_gb"], st["stamp"])
        lp.set_depth_frustum(st["sid"], dc.FOV_W, dc.FOV_V, dc.D_MIN, dc.D_MAX, st["m2s"])


def worker(args):
    from dddmr_navigation_amd import configs, depth_layer, marking
    from dddmr_navigation_amd.local_planner import LocalPlanner, RolloutError
    import depth_clear_cases as dc
    import depth_mark_cases as mc
    case, ups, ground, static, sc = scene(args.ground)
    no_map = np.zeros((0, 3), np.float32)
    theory = [configs.bench_theory("C2")]

    def depth_sources(lp):
        for i in range(case.cams):
            lp.set_depth_source(case.first_source + i, dc.Z_MIN, dc.Z_MAX, 0, max_frame_points=case.width * case.height, max_frames=1)

    def depth_cfg():
        return depth_layer.shipped_config(max_markings=case.max_markings, max_cluster_points=case.max_cluster_points, **case.layer_kw())

    times, host_min, resyncs, changed = [], [], 0, []
    if args.worker == "parent":
        with LocalPlanner(theory, max_points=200_000) as la, LocalPlanner(theory, max_points=200_000) as ld:
            depth_sources(ld)
            ml = marking.MarkingLayer(la, sc.marking_config(), ground, no_map)
            dl = depth_layer.DepthLayer(ld, depth_cfg(), ground, no_map)
            for i in range(args.warmup + args.passes):
                u = ups[i % len(ups)]
                for st in u["feeds"]:
                    feed(la if st["kind"] == "lidar" else ld, st)
                t0 = time.perf_counter()
                ml.update(mc.TBS_LIDAR, u["t_gb"])
                a, al = ml.dgraph(), ml.lethal()
                dl.update(u["t_gb"])
                d, dle = dl.dgraph(), dl.lethal()
                t1 = time.perf_counter()
                v = np.full(len(a), 99999.9)
                for x in (static, a, d):
                    v = np.where(x < v, x, v)
                mask = (al.astype(np.uint8) << 1) | (dle.astype(np.uint8) << 2)
                t2 = time.perf_counter()
                if i >= args.warmup:
                    times.append(t1 - t0)
                    host_min.append(t2 - t1)
            del v, mask
    else:
        from dddmr_navigation_amd.stack import PerceptionStack
        with LocalPlanner(theory, max_points=200_000) as lp:
            depth_sources(lp)
            ml = marking.MarkingLayer(lp, sc.marking_config(), ground, no_map)
            dl = depth_layer.DepthLayer(lp, depth_cfg(), ground, no_map)
            stack = PerceptionStack(lp, ml, dl, [static], order=sc.ORDER, max_changes=args.max_changes)
            for i in range(args.warmup + args.passes):
                u = ups[i % len(ups)]
                for st in u["feeds"]:
                    feed(lp, st)
                t0 = time.perf_counter()
                s = stack.update(mc.TBS_LIDAR, u["t_gb"])
                try:
                    stack.changes()
                except RolloutError:
                    stack.min_dgraph(), stack.lethal_mask()
                    resyncs += i >= args.warmup
                t1 = time.perf_counter()
                if i >= args.warmup:
                    times.append(t1 - t0)
                    changed.append(int(s.n_changed))
    ms = sorted(1e3 * t for t in times)
    out = {"worker": args.worker, "ground": args.ground, "n_ground": len(ground), "passes": len(ms), "median_ms": statistics.median(ms),
           "p10_ms": ms[len(ms) // 10], "p90_ms": ms[(9 * len(ms)) // 10]}
    if host_min:
        out["host_min_median_ms"] = 1e3 * statistics.median(host_min)
    if changed:
        out.update(changed_median=statistics.median(changed), changed_max=max(changed), resyncs=resyncs)
    print("RESULT " + json.dumps(out), flush=True)


def run_worker(which, ground, lib, args):
    env = dict(os.environ)
    if lib:
        env["DDDMR_LIB_NAME"] = lib
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", which, "--ground", ground, "--passes", str(args.passes), "--warmup", str(args.warmup),
           "--max-changes", str(args.max_changes)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.worker_timeout)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"worker {which} / {ground} ended with {p.returncode}")       # nothing more is started on the GPU
    line = next(l for l in p.stdout.splitlines() if l.startswith("RESULT "))
    return json.loads(line[7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", choices=["parent", "new"])
    ap.add_argument("--ground", choices=["small", "large"], default="small")
    ap.add_argument("--parent-lib", help="file name of the parent commit's library beside the new one")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--passes", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--max-changes", type=int, default=4096)
    ap.add_argument("--worker-timeout", type=int, default=240)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    if not args.parent_lib:
        ap.error("--parent-lib is required")
    report = {"protocol": "host clock around one pass, median of %d passes per round, %d alternations of the parent's and the new "
                          "library in child processes on one box; spread = range of the rounds' medians" % (args.passes, args.rounds),
              "grounds": {}}
    for ground in ("small", "large"):
        rounds = {"parent": [], "new": []}
        for r in range(args.rounds):
            rounds["parent"].append(run_worker("parent", ground, args.parent_lib, args))
            rounds["new"].append(run_worker("new", ground, None, args))
            print(ground, r, "parent %.3f ms (+ host min %.3f ms)" % (rounds["parent"][-1]["median_ms"], rounds["parent"][-1]["host_min_median_ms"]),
                  "new %.3f ms" % rounds["new"][-1]["median_ms"], flush=True)
        fig = {}
        for k, rs in rounds.items():
            med = [x["median_ms"] for x in rs]
            fig[k] = {"median_ms": statistics.median(med), "spread_ms": max(med) - min(med), "rounds": rs}
        p, n = fig["parent"], fig["new"]
        fig["bar"] = ("new < parent - parent's spread" if ground == "large" else "new <= parent + parent's spread")
        fig["bar_met"] = bool(n["median_ms"] < p["median_ms"] - p["spread_ms"]) if ground == "large" else bool(n["median_ms"] <= p["median_ms"] + p["spread_ms"])
        report["grounds"][ground] = fig
        print(ground, "parent %.3f +- %.3f ms, new %.3f +- %.3f ms, bar met: %s" % (p["median_ms"], p["spread_ms"], n["median_ms"], n["spread_ms"], fig["bar_met"]),
              flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
