#!/usr/bin/env python3
"""Time of a plan of the pre-graph global planner on the device graph, beside what a host planner pays today.

  python tools/global_plan_bench.py --parent-lib libdddmr_rollout_parent.so --out profiles/r27_global_plan.json

The scene is tools/mcl_measure_bench.py's hall: its 100 000-point ground and, as the map, the hall's 100 000 structure points
(walls and boxes; the 200 000-point map of tools/static_layer_bench.py also holds the ground itself, which puts an obstacle
at distance 0 from every node: nothing could be planned on it), with the shipped parameters (radius 1.5, inscribed_radius
0.5, inflation_descending_rate 2.0, turning_weight 0.1, a_star_expanding_radius 0.5).  The static dGraph is bound into a
host slot of the stack and the planner reads the stack's minimum (dgraph_source 0).  Workers, each a child process of its
own under its own time limit:
  plan   (the new library) global_plan_plan for a 2 m look-ahead re-plan (the DWA planner's 10 Hz case) and a plan across
         the hall, batches of 1, 4 and 16 of the re-plan; nearest and probe of 64 points; what a host planner pays on the
         parent: static_layer_get_graph + stack_get_min_dgraph of the same state; and a host A* in C++ on the downloaded
         arrays (tools/global_plan_host_astar.cpp, -O2: std::set, std::unordered_map, Initial() per plan -- this tool's
         own RESTATEMENT, not the reference, which cannot be built here)
  tick   (both libraries) the C3 tick
  stack  (both libraries) tools/stack_bench.py's `new` worker at its small ground
  cloud  (--cloud) global_plan_plan_on_cloud, the default A* on the ground cloud with its line of sight, for the same three
         queries and 16 re-plans in one call, with --inscribed as the planner's inscribed_radius and the ground nodes whose
         dGraph value is below --lethal-below as the lethal cloud; global_plan_plan on the same queries and state as the
         per-expansion yardstick (with the parent's library too); and a host A* in C++ on downloaded arrays
         (tools/global_plan_cloud_host_astar.cpp: uniform-grid searches, std::set -- this tool's own RESTATEMENT)
           python tools/global_plan_bench.py --cloud --parent-lib libdddmr_rollout_parent.so --out profiles/r29_global_plan_cloud.json
The parent's library is built from the parent commit (`make OUT=libdddmr_rollout_parent.so` there, copied beside the new
one; selected through DDDMR_LIB_NAME) and alternates with the new one --rounds times on one box.  Host clock around the
call, p10 / median / p90 of --passes calls after --warmup untimed ones.  No time is fixed in advance for a plan; the tick's
and stack_update's new medians have to lie inside the parent's own p10 - p90 spread."""
import argparse
import json
import os
import shutil
import statistics
import struct
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402


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


def host_astar(graph, ground, dgraph, cfg, starts, goals, reps):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        return None
    with tempfile.TemporaryDirectory() as tmp:
        exe, data = os.path.join(tmp, "host_astar"), os.path.join(tmp, "arrays.bin")
        subprocess.check_call([cxx, "-x", "c++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "dddmr_navigation_amd", "csrc"),
                               os.path.join(ROOT, "tools", "global_plan_host_astar.cpp"), "-o", exe])
        with open(data, "wb") as f:
            f.write(struct.pack("<IQI4d", len(ground), len(graph["neighbour"]), len(starts), cfg.turning_weight, cfg.a_star_expanding_radius,
                                cfg.inscribed_radius, cfg.inflation_descending_rate))
            for a, t in ((graph["row_start"], np.uint32), (graph["neighbour"], np.uint32), (graph["weight"], np.float32), (ground, np.float32),
                         (dgraph, np.float64), (starts, np.uint32), (goals, np.uint32)):
                f.write(np.ascontiguousarray(a, dtype=t).tobytes())
        out = subprocess.run([exe, data, str(reps)], capture_output=True, text=True, timeout=600)
        if out.returncode != 0:
            return None
        rows = [l.split() for l in out.stdout.splitlines() if l.startswith("Q ")]
        return [{"path_len": int(r[2]), "n_expanded": int(r[3]), "p10_us": float(r[4]), "median_us": float(r[5]), "p90_us": float(r[6])} for r in rows]


def cloud_host_astar(ground, dgraph, lethal, cfg, starts, goals, reps):
    """tools/global_plan_cloud_host_astar.cpp on downloaded arrays -> per query figures, None without a compiler"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        return None
    with tempfile.TemporaryDirectory() as tmp:
        exe, data = os.path.join(tmp, "cloud_host_astar"), os.path.join(tmp, "arrays.bin")
        subprocess.check_call([cxx, "-x", "c++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "dddmr_navigation_amd", "csrc"),
                               os.path.join(ROOT, "tools", "global_plan_cloud_host_astar.cpp"), "-o", exe])
        with open(data, "wb") as f:
            f.write(struct.pack("<III4d", len(ground), len(lethal), len(starts), cfg.turning_weight, cfg.a_star_expanding_radius, cfg.inscribed_radius,
                                cfg.inflation_descending_rate))
            for a, t in ((ground, np.float32), (dgraph, np.float64), (lethal, np.float32), (starts, np.uint32), (goals, np.uint32)):
                f.write(np.ascontiguousarray(a, dtype=t).tobytes())
        out = subprocess.run([exe, data, str(reps)], capture_output=True, text=True, timeout=600)
        if out.returncode != 0:
            return None
        rows = [l.split() for l in out.stdout.splitlines() if l.startswith("Q ")]
        return [{"path_len": int(r[2]), "n_expanded": int(r[3]), "n_los_tested": int(r[4]), "p10_us": float(r[5]), "median_us": float(r[6]), "p90_us": float(r[7])}
                for r in rows]


def cloud_worker(args, out):
    """--cloud: plan_on_cloud beside global_plan_plan on the same queries and state, and the host restatement.  With
    DDDMR_LIB_NAME set (the parent's library, which has no plan_on_cloud) only global_plan_plan is timed."""
    import mcl_measure_bench as mb
    from dddmr_navigation_amd import configs, global_plan, stack, static_layer
    from dddmr_navigation_amd.local_planner import LocalPlanner
    parent_only = "DDDMR_LIB_NAME" in os.environ
    _, ground, _, structure = mb.hall(np.random.default_rng(15))
    structure = structure.astype(np.float32)
    out.update(n_ground=len(ground), n_map=len(structure), inscribed_radius=args.inscribed, lethal_below=args.lethal_below)
    with LocalPlanner([configs.bench_theory("C2")], max_points=1 << 16) as lp:
        sl = static_layer.StaticLayer(lp, static_layer.shipped_config(max_ground_points=mb.N_GROUND, max_map_points=mb.N_MAP, max_edges=1 << 24))
        sl.build(ground, structure)
        ps = stack.PerceptionStack(lp, host_layers=(None,), n_ground=len(ground))
        sl.bind(0, 0)
        ps.update()
        cfg = global_plan.shipped_config(max_open_entries=1 << 20, max_expansions=mb.N_GROUND, inscribed_radius=args.inscribed)
        gp = global_plan.GlobalPlan(lp, cfg, mb.N_GROUND)
        dgraph = ps.min_dgraph()
        free = dgraph[:-1] >= 0.5                                               # (the queries of the plan worker)
        lethal = ground[dgraph[:-1] < args.lethal_below]                        # the ground nodes at the scene's obstacles
        out.update(free_nodes=int(free.sum()), n_lethal=len(lethal))
        at = lambda x, y: int(np.argmin(np.where(free, np.hypot(ground[:, 0] - x, ground[:, 1] - y), np.inf)))
        queries = {"replan_2m": (at(0.0, 0.0), at(2.0, 0.0)), "across_20m": (at(-10.0, -10.0), at(6.0, 2.0)), "across_hall": (at(-45.0, -45.0), at(45.0, 45.0))}

        def series(fn, key):
            res = {}
            for name, (s, g) in queries.items():
                r = fn(s, g)
                t0 = time.perf_counter()
                fn(s, g)
                one = time.perf_counter() - t0
                passes = int(min(args.passes, max(5, 10.0 / max(one, 1e-6))))      # (a long search: fewer calls, at most about 10 s of them)
                t = figures(timed(lambda: fn(s, g), passes, min(args.warmup, passes)), 1e6)
                res[name] = {"start": s, "goal": g, "status": r.status, "path_len": int(len(r.path)), "n_expanded": r.n_expanded, "n_pushed": r.n_pushed,
                             "us": t, "us_per_expansion": t["median"] / max(r.n_expanded, 1)}
                for k in key:
                    res[name][k] = int(getattr(r, k))
            return res
        out["pre_graph"] = series(gp.plan, ())
        if not parent_only:
            t0 = time.perf_counter()
            gp.set_lethal_points(lethal)
            out["set_lethal_points_us"] = (time.perf_counter() - t0) * 1e6
            out["cloud"] = series(gp.plan_on_cloud, ("n_knn_fallbacks", "n_lethal_skipped", "n_los_tested", "n_los_blocked", "n_los_capped", "max_successors"))
            s, g = queries["replan_2m"]
            out["cloud_batch_us"] = {str(n): figures(timed(lambda: gp.plan_many_on_cloud([s] * n, [g] * n), args.passes, args.warmup), 1e6) for n in (1, 16)}
            # what a host planner needs before it can plan: the stacked dGraph (the lethal cloud it aggregates on the host anyway)
            out["get_min_dgraph_us"] = figures(timed(ps.min_dgraph, args.passes, args.warmup), 1e6)
            out["get_lethal_nodes_us"] = figures(timed(ps.lethal_nodes, args.passes, args.warmup), 1e6)
    if not parent_only:
        names = list(queries)
        host = cloud_host_astar(ground, dgraph, lethal, cfg, [queries[k][0] for k in names], [queries[k][1] for k in names], 5)
        out["host_astar"] = None if host is None else dict(zip(names, host))
        out["host_astar_label"] = ("tools/global_plan_cloud_host_astar.cpp, g++ -O2: this tool's restatement with uniform-grid searches, std::set / "
                                   "std::unordered_map and Initial() per plan, the lethal grid built outside the timed plan; not the reference")
    print("RESULT " + json.dumps(out), flush=True)


def worker(args):
    out = {"worker": args.worker}
    if args.worker == "cloud":
        return cloud_worker(args, out)
    from dddmr_navigation_amd import configs, scenes
    from dddmr_navigation_amd.local_planner import LocalPlanner
    if args.worker == "tick":
        sc = scenes.bench_scene("C3")
        with LocalPlanner([sc.theory], max_points=max(len(sc.cloud), 1)) as lp:
            lp.set_cloud(sc.cloud)
            lp.setPlan(sc.plan)
            name = sc.theory.name.decode()
            out["tick_us"] = figures(timed(lambda: lp.tick(name, sc.tick), args.passes, args.warmup), 1e6)
        print("RESULT " + json.dumps(out), flush=True)
        return
    import mcl_measure_bench as mb
    from dddmr_navigation_amd import global_plan, stack, static_layer
    _, ground, _, structure = mb.hall(np.random.default_rng(15))
    structure = structure.astype(np.float32)
    out.update(n_ground=len(ground), n_map=len(structure))
    with LocalPlanner([configs.bench_theory("C2")], max_points=1 << 16) as lp:
        sl = static_layer.StaticLayer(lp, static_layer.shipped_config(max_ground_points=mb.N_GROUND, max_map_points=mb.N_MAP, max_edges=1 << 24))
        st = sl.build(ground, structure)
        out["build"] = {k: int(getattr(st, k)) for k, _ in st._fields_}
        ps = stack.PerceptionStack(lp, host_layers=(None,), n_ground=len(ground))
        sl.bind(0, 0)
        ps.update()
        cfg = global_plan.shipped_config(max_open_entries=1 << 20, max_expansions=mb.N_GROUND)
        gp = global_plan.GlobalPlan(lp, cfg, mb.N_GROUND)
        dgraph = ps.min_dgraph()
        free = dgraph[:-1] >= cfg.inscribed_radius
        out["free_nodes"] = int(free.sum())
        at = lambda x, y: int(np.argmin(np.where(free, np.hypot(ground[:, 0] - x, ground[:, 1] - y), np.inf)))
        queries = {"replan_2m": (at(0.0, 0.0), at(2.0, 0.0)), "across_20m": (at(-10.0, -10.0), at(6.0, 2.0)), "across_hall": (at(-45.0, -45.0), at(45.0, 45.0))}
        out["plans"] = {}
        for name, (s, g) in queries.items():
            r = gp.plan(s, g)
            t0 = time.perf_counter()
            gp.plan(s, g)
            one = time.perf_counter() - t0
            passes = int(min(args.passes, max(5, 20.0 / max(one, 1e-6))))      # (a long search: fewer calls, at most about 20 s of them)
            t = figures(timed(lambda: gp.plan(s, g), passes, min(args.warmup, passes)), 1e6)
            out["plans"][name] = {"start": s, "goal": g, "status": r.status, "path_len": int(len(r.path)), "n_expanded": r.n_expanded, "n_pushed": r.n_pushed,
                                  "n_discarded_closed": r.n_discarded_closed, "us": t, "us_per_expansion": t["median"] / max(r.n_expanded, 1)}
        s, g = queries["replan_2m"]
        out["batch_us"] = {str(n): figures(timed(lambda: gp.plan_many([s] * n, [g] * n), args.passes, args.warmup), 1e6) for n in (1, 4, 16)}
        pts = ground[:: len(ground) // 64][:64]
        out["nearest_64_us"] = figures(timed(lambda: gp.nearest(pts), args.passes, args.warmup), 1e6)
        out["probe_64_us"] = figures(timed(lambda: gp.probe(pts), args.passes, args.warmup), 1e6)
        # what a host planner pays on the parent for the same state: the graph after a regeneration, the dGraph after a pass
        out["get_graph_ms"] = figures(timed(sl.graph, max(args.passes // 20, 5), 2), 1e3)
        out["get_min_dgraph_us"] = figures(timed(ps.min_dgraph, args.passes, args.warmup), 1e6)
        graph = sl.graph()
        out["graph_bytes"] = int(sum(graph[k].nbytes for k in graph))
    names = list(queries)
    host = host_astar(graph, ground, dgraph, cfg, [queries[k][0] for k in names], [queries[k][1] for k in names], 5)
    out["host_astar"] = None if host is None else dict(zip(names, host))
    out["host_astar_label"] = "tools/global_plan_host_astar.cpp, g++ -O2: this tool's restatement with std::set / std::unordered_map and Initial() per plan, not the reference"
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


def main_cloud(args, me):
    cloud = run_child(me + ["cloud"], None, args.worker_timeout)
    report = {"protocol": "host clock around the call, p10 / median / p90 of up to %d calls after %d untimed ones, every worker a child process under its own "
                          "time limit; the tick, stack_update and global_plan_plan with the parent's and the new library alternating, %d rounds"
                          % (args.passes, args.warmup, args.rounds), "cloud": cloud}
    for k, v in cloud["cloud"].items():
        h, p = (cloud.get("host_astar") or {}).get(k), cloud["pre_graph"][k]
        print("%s: plan_on_cloud %d expansions, %d marched edges, %.1f us (%.2f us per expansion); global_plan_plan %d expansions, %.1f us (%.2f)%s"
              % (k, v["n_expanded"], v["n_los_tested"], v["us"]["median"], v["us_per_expansion"], p["n_expanded"], p["us"]["median"], p["us_per_expansion"],
                 "" if not h else "; host restatement %d expansions, %.1f us" % (h["n_expanded"], h["median_us"])), flush=True)
    print("16 re-plans in one call %.1f us; get_min_dgraph %.1f us" % (cloud["cloud_batch_us"]["16"]["median"], cloud["get_min_dgraph_us"]["median"]), flush=True)
    if args.parent_lib:
        rounds = {"parent": [], "new": []}
        stack_cmd = [sys.executable, os.path.join(ROOT, "tools", "stack_bench.py"), "--worker", "new", "--ground", "small", "--passes", str(args.passes),
                     "--warmup", str(args.warmup)]
        for _ in range(args.rounds):
            for which, lib in (("parent", args.parent_lib), ("new", None)):
                rounds[which].append({"tick": run_child(me + ["tick"], lib, args.worker_timeout), "stack": run_child(stack_cmd, lib, args.worker_timeout),
                                      "plan": run_child(me + ["cloud"], lib, args.worker_timeout)["pre_graph"] if lib else None})
        for r in rounds["new"]:
            r["plan"] = cloud["pre_graph"]                                      # (the new library's global_plan_plan: the cloud worker's own figures)
        report["inside_parent_spread"] = {}
        getters = [("tick_C3_us", lambda r, k: r["tick"]["tick_us"][k]), ("stack_update_small_ms", lambda r, k: r["stack"][k + "_ms"])]
        getters += [("global_plan_plan_%s_us" % q, (lambda q: lambda r, k: r["plan"][q]["us"][k])(q)) for q in cloud["pre_graph"]]
        for name, get in getters:
            new = statistics.median(get(r, "median") for r in rounds["new"])
            lo, hi = (statistics.median(get(r, k) for r in rounds["parent"]) for k in ("p10", "p90"))
            report["inside_parent_spread"][name] = {"new_median": new, "parent_median": statistics.median(get(r, "median") for r in rounds["parent"]),
                                                    "parent_p10": lo, "parent_p90": hi, "inside": bool(lo <= new <= hi)}
            print(name, report["inside_parent_spread"][name], flush=True)
        report["rounds"] = rounds
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", choices=["plan", "tick", "cloud"])
    ap.add_argument("--cloud", action="store_true", help="time global_plan_plan_on_cloud (the default A* on the ground cloud) instead of the pre-graph plan")
    ap.add_argument("--inscribed", type=float, default=0.15, help="--cloud: the planner's inscribed_radius (at the shipped 0.5 no radius-search edge is long enough to be marched)")
    ap.add_argument("--lethal-below", type=float, default=0.25, help="--cloud: ground nodes whose dGraph value is below this are the lethal cloud")
    ap.add_argument("--parent-lib", help="file name of the parent commit's library beside the new one")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--passes", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--worker-timeout", type=int, default=300)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    me = [sys.executable, os.path.abspath(__file__), "--passes", str(args.passes), "--warmup", str(args.warmup), "--inscribed", str(args.inscribed),
          "--lethal-below", str(args.lethal_below), "--worker"]
    if args.cloud:
        return main_cloud(args, me)
    plan = run_child(me + ["plan"], None, args.worker_timeout)
    report = {"protocol": "host clock around the call, p10 / median / p90 of %d calls after %d untimed ones, every worker a child process under its own "
                          "time limit; the tick and stack_update with the parent's and the new library alternating, %d rounds" % (args.passes, args.warmup, args.rounds),
              "plan": plan}
    for k, v in plan["plans"].items():
        h = (plan.get("host_astar") or {}).get(k)
        print("%s: %d expansions, device %.1f us (%.2f us per expansion)%s" % (k, v["n_expanded"], v["us"]["median"], v["us_per_expansion"],
                                                                               "" if not h else ", host restatement %.1f us" % h["median_us"]), flush=True)
    print("get_graph %.2f ms, get_min_dgraph %.1f us" % (plan["get_graph_ms"]["median"], plan["get_min_dgraph_us"]["median"]), flush=True)
    if args.parent_lib:
        rounds = {"parent": [], "new": []}
        stack_cmd = [sys.executable, os.path.join(ROOT, "tools", "stack_bench.py"), "--worker", "new", "--ground", "small", "--passes", str(args.passes),
                     "--warmup", str(args.warmup)]
        for _ in range(args.rounds):
            for which, lib in (("parent", args.parent_lib), ("new", None)):
                rounds[which].append({"tick": run_child(me + ["tick"], lib, args.worker_timeout), "stack": run_child(stack_cmd, lib, args.worker_timeout)})
        med = lambda rs, a, b: statistics.median(r[a][b] if not isinstance(r[a].get(b), dict) else r[a][b] for r in rs)
        report["inside_parent_spread"] = {}
        for name, get in (("tick_C3_us", lambda r, k: r["tick"]["tick_us"][k]), ("stack_update_small_ms", lambda r, k: r["stack"][k + "_ms"])):
            new = statistics.median(get(r, "median") for r in rounds["new"])
            lo, hi = (statistics.median(get(r, k) for r in rounds["parent"]) for k in ("p10", "p90"))
            report["inside_parent_spread"][name] = {"new_median": new, "parent_median": statistics.median(get(r, "median") for r in rounds["parent"]),
                                                    "parent_p10": lo, "parent_p90": hi, "inside": bool(lo <= new <= hi)}
            print(name, report["inside_parent_spread"][name], flush=True)
        report["rounds"] = rounds
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
