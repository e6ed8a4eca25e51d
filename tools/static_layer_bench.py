#!/usr/bin/env python3
"""Time of a static-layer regeneration on the device, beside what it replaces, and of stack_update and mcl_measure after it.

  python tools/static_layer_bench.py --parent-lib libdddmr_rollout_parent.so --out profiles/r26_static_layer.json

The scene is tools/mcl_measure_bench.py's hall: a 100 000-point ground and a 200 000-point map, with the shipped
parameters of p2p_move_base_localization.yaml (radius 1.5, static_imposing_radius 1.5, inscribed_radius 0.5,
max_obstacle_distance 9999).  Workers, each a child process of its own under its own time limit:
  layer    (the new library) dddmr_rollout_static_layer_build with generate_static_graph on and off, set_zones with two
           zones of 200 points, then static_layer_bind beside stack_set_host_layer of the same array
  scipy    (no device) tests/helpers/static_layer_ref.py's build() on the same inputs, once: SciPy's cKDTree plus NumPy,
           labelled as such -- NOT PCL, the reference cannot be built here
  measure  (both libraries) mcl_measure at 60 and 1024 particles on the same hall
  stack    (both libraries) tools/stack_bench.py's `new` worker: stack_update at its small and large ground
The parent's library is built from the parent commit (`make OUT=libdddmr_rollout_parent.so` there, copied beside the new
one; selected through DDDMR_LIB_NAME) and alternates with the new one --rounds times on one box.  Host clock around the
call, median and p10 / p90 of --passes calls after --warmup untimed ones.  No bar is set on the build (nothing earlier
does this work); stack_update's and mcl_measure's new medians have to lie inside the parent's own p10 - p90 spread.
For the kernels' shares:
  rocprofv3 --kernel-trace --stats -- python tools/static_layer_bench.py --worker layer --passes 20
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

PARTICLES = (60, 1024)
INFLATION = 0.5


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


def zone_points(ground):
    t = np.linspace(0.0, 1.0, 200)
    a = np.stack([-20.0 + 10.0 * t, 5.0 + 0.0 * t, 0.0 * t], axis=1)
    b = np.stack([10.0 + 0.0 * t, -30.0 + 8.0 * t, 0.0 * t], axis=1)
    return np.concatenate([a, b]).astype(np.float32)


def worker(args):
    import mcl_measure_bench as mb
    out = {"worker": args.worker}
    if args.worker == "scipy":
        import static_layer_ref as R
        static_map, ground = mb.scene(PARTICLES[0])[:2]
        t0 = time.perf_counter()
        ref = R.build(ground, static_map, R.config())
        out["host_scipy_build_s"] = time.perf_counter() - t0
        out["n_edges"] = int(len(ref["neighbour"]))
        print("RESULT " + json.dumps(out), flush=True)
        return
    from dddmr_navigation_amd import configs, localization
    from dddmr_navigation_amd.local_planner import LocalPlanner
    scenes = {n: mb.scene(n) for n in PARTICLES}
    static_map, ground = scenes[PARTICLES[0]][:2]
    out.update(n_map=len(static_map), n_ground=len(ground))
    with LocalPlanner([configs.bench_theory("C2")], max_points=1 << 16) as lp:
        if args.worker == "layer":
            from dddmr_navigation_amd import stack, static_layer
            for key, graph in (("graph_on", 1), ("graph_off", 0)):
                sl = static_layer.StaticLayer(lp, static_layer.shipped_config(max_ground_points=mb.N_GROUND, max_map_points=mb.N_MAP, max_edges=1 << 24,
                                                                               generate_static_graph=graph))
                out["build_ms_" + key] = figures(timed(lambda: sl.build(ground, static_map), args.passes, args.warmup), 1e3)
                out["build_stats_" + key] = {k: int(getattr(sl.last, k)) for k, _ in sl.last._fields_}
            zones = zone_points(ground)
            out["set_zones_ms"] = figures(timed(lambda: sl.set_zones(zones, INFLATION), args.passes, args.warmup), 1e3)
            out["set_zones_stats"] = {k: int(getattr(sl.last, k)) for k, _ in sl.last._fields_}
            st = stack.PerceptionStack(lp, host_layers=(None, None), n_ground=len(ground))
            values = sl.dgraph()
            out["bind_us"] = figures(timed(lambda: sl.bind(0, 0), args.passes, args.warmup), 1e6)
            out["stack_set_host_layer_us"] = figures(timed(lambda: st.set_host_layer(1, values), args.passes, args.warmup), 1e6)
        else:
            pm = localization.ParticleMeasure(lp, localization.shipped_config(max_map_points=mb.N_MAP, max_ground_points=mb.N_GROUND, max_particles=max(PARTICLES)))
            pm.set_map(static_map, ground, scenes[PARTICLES[0]][2])
            out["measure_us"] = {}
            for n in PARTICLES:
                flat, ls, states = scenes[n][3:]
                out["measure_us"][str(n)] = figures(timed(lambda: pm.measure(flat, ls, states), args.passes, args.warmup), 1e6)
    print("RESULT " + json.dumps(out), flush=True)


def run_child(cmd, lib, timeout):
    env = dict(os.environ)
    if lib:
        env["DDDMR_LIB_NAME"] = lib
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"{' '.join(cmd[1:4])} ended with {p.returncode}")       # nothing more is started on the GPU
    return json.loads(next(l for l in p.stdout.splitlines() if l.startswith("RESULT "))[7:])


def run_worker(which, lib, args):
    return run_child([sys.executable, os.path.abspath(__file__), "--worker", which, "--passes", str(args.passes), "--warmup", str(args.warmup)], lib,
                     args.worker_timeout)


def run_stack(ground, lib, args):
    return run_child([sys.executable, os.path.join(ROOT, "tools", "stack_bench.py"), "--worker", "new", "--ground", ground, "--passes", str(args.passes),
                      "--warmup", str(args.warmup)], lib, args.worker_timeout)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", choices=["layer", "scipy", "measure"])
    ap.add_argument("--parent-lib", help="file name of the parent commit's library beside the new one")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--passes", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--worker-timeout", type=int, default=240)
    ap.add_argument("--skip-scipy", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    if not args.parent_lib:
        ap.error("--parent-lib is required")
    med = lambda rs, *path: statistics.median(_dig(x, path) for x in rs)
    layer = [run_worker("layer", None, args) for _ in range(args.rounds)]
    report = {"protocol": "host clock around the call, median and p10 / p90 of %d calls after %d untimed ones per round, %d rounds in child processes on one "
                          "box (the parent's and the new library alternating where both run); a figure below is the median over the rounds" % (
                              args.passes, args.warmup, args.rounds),
              "shape": {"n_ground": layer[0]["n_ground"], "n_map": layer[0]["n_map"], "radius_of_ground_connection": 1.5, "static_imposing_radius": 1.5,
                        "inscribed_radius": 0.5, "max_obstacle_distance": 9999.0, "zone_points": 400, "inflation_distance": INFLATION}}
    for key in ("build_ms_graph_on", "build_ms_graph_off", "set_zones_ms", "bind_us", "stack_set_host_layer_us"):
        report[key] = {k: med(layer, key, k) for k in ("median", "p10", "p90")}
    for key in ("build_stats_graph_on", "build_stats_graph_off", "set_zones_stats"):
        report[key] = layer[-1][key]
    print("build: graph on %.3f ms, off %.3f ms; set_zones %.3f ms; bind %.1f us, stack_set_host_layer %.1f us" % (
        report["build_ms_graph_on"]["median"], report["build_ms_graph_off"]["median"], report["set_zones_ms"]["median"], report["bind_us"]["median"],
        report["stack_set_host_layer_us"]["median"]), flush=True)
    rounds = {"parent": [], "new": []}
    for r in range(args.rounds):
        for which, lib in (("parent", args.parent_lib), ("new", None)):
            rounds[which].append({"measure": run_worker("measure", lib, args), "stack_small": run_stack("small", lib, args),
                                  "stack_large": run_stack("large", lib, args)})
    report["inside_parent_spread"] = {}
    checks = [("mcl_measure_%s_us" % n, ("measure", "measure_us", n), ("median", "p10", "p90")) for n in map(str, PARTICLES)]
    checks += [("stack_update_%s_ms" % g, ("stack_" + g,), ("median_ms", "p10_ms", "p90_ms")) for g in ("small", "large")]
    for name, path, (km, k10, k90) in checks:
        new = med(rounds["new"], *path, km)
        lo, hi = med(rounds["parent"], *path, k10), med(rounds["parent"], *path, k90)
        report["inside_parent_spread"][name] = {"new_median": new, "parent_median": med(rounds["parent"], *path, km), "parent_p10": lo, "parent_p90": hi,
                                                "inside": bool(lo <= new <= hi)}
        print("%s: new %.3f, parent %.3f (p10 %.3f, p90 %.3f), inside: %s" % (name, new, report["inside_parent_spread"][name]["parent_median"], lo, hi,
                                                                              lo <= new <= hi), flush=True)
    if not args.skip_scipy:
        host = run_child([sys.executable, os.path.abspath(__file__), "--worker", "scipy"], None, 900)
        report["host_scipy_ckdtree_build_s"] = host["host_scipy_build_s"]
        report["host_label"] = "tests/helpers/static_layer_ref.py build(): SciPy cKDTree candidates + NumPy decisions, one call, not PCL"
        report["host_n_edges"] = host["n_edges"]
        print("SciPy restatement: %.1f s, %d edges" % (host["host_scipy_build_s"], host["n_edges"]), flush=True)
    report["rounds"] = {"layer": layer, **rounds}
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
