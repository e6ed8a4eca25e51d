#!/usr/bin/env python3
"""Time of a sub-map warm-up on the device, beside what it replaces, and of mcl_measure after it.

  python tools/submap_bench.py --parent-lib libdddmr_rollout_parent.so --out profiles/r25_submap.json

The scene is tools/mcl_measure_bench.py's hall (a 200 000-point map, a 100 000-point ground) cut into 60 keyframes of
10 m x 16.7 m.  new: the keyframes go into the store once (not timed), then dddmr_rollout_submap_warm_up over all 60 ids
is timed, then a swap and mcl_measure at 60 and 1024 particles.  parent (a library built from the parent commit:
`make OUT=libdddmr_rollout_parent.so` there, copied beside the new one; selected through DDDMR_LIB_NAME): the normals
come from the host -- SciPy's cKDTree.query(k=20) plus the NumPy normals of tests/helpers/mcl_observation_ref.py, timed
and labelled as such (NOT PCL: the reference cannot be built here) -- then mcl_set_map on the same arrays is timed (the
upload and the grids a warm-up replaces, not the normals), then mcl_measure on that map.

Every measurement runs in a child process of its own (`--worker`), the two libraries alternate --rounds times on one box;
host clock around the call, median and p10 / p90 of --passes calls after --warmup untimed ones.  There is no bar on the
warm-up (nothing earlier does this work); mcl_measure's new median has to lie inside the parent's own p10 - p90 spread.
For the k-NN kernel's share:
  rocprofv3 --kernel-trace --stats -- python tools/submap_bench.py --worker new --passes 50
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

TILES = (10, 6)
PARTICLES = (60, 1024)


def keyframes(static_map, ground):
    """the hall cut into TILES keyframes: -> [(corner, ground, position)] and the concatenation in id order"""
    def tile(p):
        ix = np.clip(((p[:, 0] + 50.0) / (100.0 / TILES[0])).astype(int), 0, TILES[0] - 1)
        iy = np.clip(((p[:, 1] + 50.0) / (100.0 / TILES[1])).astype(int), 0, TILES[1] - 1)
        return ix * TILES[1] + iy
    tm, tg = tile(static_map), tile(ground)
    kfs = []
    for t in range(TILES[0] * TILES[1]):
        pos = (-50.0 + (t // TILES[1] + 0.5) * 100.0 / TILES[0], -50.0 + (t % TILES[1] + 0.5) * 100.0 / TILES[1], 0.0)
        kfs.append((static_map[tm == t], ground[tg == t], pos))
    return kfs, np.concatenate([k[0] for k in kfs]), np.concatenate([k[1] for k in kfs])


def figures(times, unit):
    v = sorted(unit * t for t in times)
    return {"calls": len(v), "median": statistics.median(v), "p10": v[len(v) // 10], "p90": v[(9 * len(v)) // 10]}


def timed(fn, passes, warmup):
    out = []
    for i in range(warmup + passes):
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        if i >= warmup:
            out.append(t1 - t0)
    return out


def worker(args):
    import mcl_measure_bench as mb
    import mcl_observation_ref as R
    from dddmr_navigation_amd import configs, localization
    from dddmr_navigation_amd.local_planner import LocalPlanner
    scenes = {n: mb.scene(n) for n in PARTICLES}
    static_map, ground = scenes[PARTICLES[0]][:2]
    kfs, cat_map, cat_ground = keyframes(static_map, ground)
    out = {"worker": args.worker, "n_keyframes": len(kfs), "n_map": len(cat_map), "n_ground": len(cat_ground)}
    with LocalPlanner([configs.bench_theory("C2")], max_points=1 << 16) as lp:
        pm = localization.ParticleMeasure(lp, localization.shipped_config(max_map_points=mb.N_MAP, max_ground_points=mb.N_GROUND, max_particles=max(PARTICLES)))
        if args.worker == "new":
            from dddmr_navigation_amd import submaps
            sm = submaps.SubMaps(lp, pm, submaps.shipped_config(max_keyframes=len(kfs), max_store_map_points=mb.N_MAP, max_store_ground_points=mb.N_GROUND))
            for c, g, pos in kfs:
                sm.add_keyframe(c, g, pos)
            ids = np.arange(len(kfs), dtype=np.int32)
            out["warm_up_ms"] = figures(timed(lambda: sm.warm_up(ids), args.passes, args.warmup), 1e3)
            st = sm.last
            out["warm_up_stats"] = {k: int(getattr(st, k)) for k, _ in st._fields_}
            sm.swap()
        else:
            from scipy.spatial import cKDTree
            host = []
            for _ in range(3):
                t0 = time.perf_counter()
                nb = cKDTree(cat_ground).query(cat_ground, k=20)[1]
                t1 = time.perf_counter()
                nrm = R.normals(cat_ground, nb)
                host.append((t1 - t0, time.perf_counter() - t1))
            out["host_scipy_knn_ms"] = 1e3 * statistics.median(h[0] for h in host)
            out["host_numpy_normals_ms"] = 1e3 * statistics.median(h[1] for h in host)
            out["set_map_ms"] = figures(timed(lambda: pm.set_map(cat_map, cat_ground, nrm), args.passes, args.warmup), 1e3)
        out["measure_us"] = {}
        for n in PARTICLES:
            flat, ls, states = scenes[n][3:]
            out["measure_us"][str(n)] = figures(timed(lambda: pm.measure(flat, ls, states), args.passes, args.warmup), 1e6)
            out["measure_us"][str(n)]["healthy"] = int(pm.terms(n)["healthy"].sum())
    print("RESULT " + json.dumps(out), flush=True)


def run_worker(which, lib, args):
    env = dict(os.environ)
    if lib:
        env["DDDMR_LIB_NAME"] = lib
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", which, "--passes", str(args.passes), "--warmup", str(args.warmup)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.worker_timeout)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"worker {which} ended with {p.returncode}")       # nothing more is started on the GPU
    return json.loads(next(l for l in p.stdout.splitlines() if l.startswith("RESULT "))[7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", choices=["parent", "new"])
    ap.add_argument("--parent-lib", help="file name of the parent commit's library beside the new one")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--passes", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--worker-timeout", type=int, default=240)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    if not args.parent_lib:
        ap.error("--parent-lib is required")
    rounds = {"parent": [], "new": []}
    for r in range(args.rounds):
        rounds["parent"].append(run_worker("parent", args.parent_lib, args))
        rounds["new"].append(run_worker("new", None, args))
        p, n = rounds["parent"][-1], rounds["new"][-1]
        print(r, "warm_up %.3f ms | parent set_map %.3f ms, SciPy k-NN %.0f ms + NumPy normals %.0f ms | measure(60) new %.1f / parent %.1f us" % (
            n["warm_up_ms"]["median"], p["set_map_ms"]["median"], p["host_scipy_knn_ms"], p["host_numpy_normals_ms"],
            n["measure_us"]["60"]["median"], p["measure_us"]["60"]["median"]), flush=True)
    med = lambda rs, *path: statistics.median(_dig(x, path) for x in rs)
    report = {"protocol": "host clock around the call, median and p10 / p90 of %d calls after %d untimed ones per round, %d alternations of the parent's "
                          "and the new library in child processes on one box; a figure below is the median over the rounds" % (args.passes, args.warmup, args.rounds),
              "warm_up_ms": {k: med(rounds["new"], "warm_up_ms", k) for k in ("median", "p10", "p90")},
              "warm_up_stats": rounds["new"][-1]["warm_up_stats"],
              "parent_set_map_ms": {k: med(rounds["parent"], "set_map_ms", k) for k in ("median", "p10", "p90")},
              "host_scipy_ckdtree_query_k20_ms": med(rounds["parent"], "host_scipy_knn_ms"),
              "host_numpy_normals_ms": med(rounds["parent"], "host_numpy_normals_ms"),
              "host_label": "SciPy cKDTree.query(k=20) + NumPy normals, not PCL",
              "measure_us": {}, "rounds": rounds}
    for n in map(str, PARTICLES):
        new = med(rounds["new"], "measure_us", n, "median")
        lo, hi = med(rounds["parent"], "measure_us", n, "p10"), med(rounds["parent"], "measure_us", n, "p90")
        report["measure_us"][n] = {"new_median": new, "parent_median": med(rounds["parent"], "measure_us", n, "median"), "parent_p10": lo,
                                   "parent_p90": hi, "new_inside_parent_spread": bool(lo <= new <= hi)}
        print("measure(%s): new %.1f us, parent %.1f us (p10 %.1f, p90 %.1f), inside: %s" % (
            n, new, report["measure_us"][n]["parent_median"], lo, hi, report["measure_us"][n]["new_inside_parent_spread"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")


def _dig(x, path):
    for k in path:
        x = x[k]
    return x


if __name__ == "__main__":
    main()
