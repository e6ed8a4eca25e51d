#!/usr/bin/env python3
"""Time of one filter step (predict, measure, resample, set_noise) of mcl_3dl's localiser at 60 / 1024 / 16 384 particles
and 100 flat + 550 less-sharp observation points in mcl_measure_bench's hall, two ways, alternating step by step in one
run:

  device   dddmr_rollout_mcl_filter_predict / _measure (the lidar model on the resident poses) / _resample / _set_noise
  host     the route of the commit before the particle set: dddmr_rollout_mcl_measure_prepared on uploaded states plus the
           host's serial loops -- tools/mcl_filter_host_step.cpp, THIS TOOL'S OWN C++ restatement of the host filter,
           not the reference's code -- including both transfers (states up, likelihoods down)

  python tools/mcl_filter_bench.py --out profiles/r30_mcl_filter.json

Host clock around each step, median and p10 / p90 of --passes steps after --warmup untimed ones.  The random numbers
of both ways are drawn before the clock starts.  Whichever way wins is reported.

--measure-only prints the statistics of dddmr_rollout_mcl_measure_prepared alone as one JSON line: run it once with the
shipped library and once with DDDMR_LIB_NAME naming a build of the parent commit to see that the measure stayed inside
the parent's own spread (--compare-with NAME does both, alternating processes, and records the result).
"""
import argparse
import ctypes as C
import json
import os
import shutil
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

F = np.float32
LIN_TC, ANG_TC, VAR_DIST, VAR_ANG = 5.0, 10.0, 2.0, 1.57


def stats_of(times):
    us = sorted(1e6 * t for t in times)
    return {"median_us": statistics.median(us), "p10_us": us[len(us) // 10], "p90_us": us[(9 * len(us)) // 10]}


def host_library():
    """tools/mcl_filter_host_step.cpp built beside itself (tools/_build/, not tracked); built once, reused"""
    src = os.path.join(ROOT, "tools", "mcl_filter_host_step.cpp")
    out = os.path.join(ROOT, "tools", "_build", "libmcl_filter_host_step.so")
    if not os.path.exists(out) or os.path.getmtime(out) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.run([shutil.which("g++") or "c++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", out, src], check=True)
    lib = C.CDLL(out)
    vp, f = C.c_void_p, C.c_float
    lib.host_predict.argtypes = [C.c_size_t, vp, vp, vp, vp, f, f, f]
    lib.host_predict.restype = None
    lib.host_update.argtypes = [C.c_size_t, vp, vp, vp, vp, vp, f, f, f, vp, vp, vp]
    lib.host_update.restype = C.c_uint32
    return lib


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def setup(lp, n):
    import mcl_measure_bench as mb
    import mcl_observation_cases as oc
    from dddmr_navigation_amd import localization
    pm = localization.ParticleMeasure(lp, localization.shipped_config(max_map_points=mb.N_MAP, max_ground_points=mb.N_GROUND,
                                                                       max_particles=max(n, 64)))
    static_map, ground, nrm, flat, ls, states = mb.scene(n)
    pm.set_map(static_map, ground, nrm)
    pm.configure_observation(localization.shipped_observation_config(max_flat_points=mb.N_FLAT, max_less_sharp_points=mb.N_LS))
    pm.prepare(oc.to_sensor(flat), oc.to_sensor(ls[:, :3]), oc.T_B2S)
    return pm, states


def draws(n, steps, rng):
    out = []
    for _ in range(steps):
        d = (rng.standard_normal((n, 6)) * np.array([0.02, 0.02, 0.02, 0.01, 0.01, 0.01])).astype(F)
        rows = np.zeros((n, 10), F)
        rows[:, 0:3], rows[:, 7:10] = d[:, 0:3], d[:, 3:6]
        h = (d[:, 3:6] / F(2)).astype(F)                       # setRPY, vectorised (the tool's inputs, not a pinned answer)
        c, s = np.cos(h).astype(F), np.sin(h).astype(F)
        rows[:, 3] = c[:, 2] * s[:, 0] * c[:, 1] - s[:, 2] * c[:, 0] * s[:, 1]
        rows[:, 4] = c[:, 2] * c[:, 0] * s[:, 1] + s[:, 2] * s[:, 0] * c[:, 1]
        rows[:, 5] = s[:, 2] * c[:, 0] * c[:, 1] - c[:, 2] * s[:, 0] * s[:, 1]
        rows[:, 6] = c[:, 2] * c[:, 0] * c[:, 1] + s[:, 2] * s[:, 0] * s[:, 1]
        z = (rng.standard_normal((n, 4)) * np.array([0.6, 0.3, 0.3, 0.6]) * 0.02).astype(F)
        out.append((float(F(rng.uniform(0, 1 - 1e-6))), rows, z))
    return out


def run_steps(n, passes, warmup):
    from dddmr_navigation_amd import configs, localization
    from dddmr_navigation_amd.local_planner import LocalPlanner
    host = host_library()
    rng = np.random.default_rng(30 + n)
    steps = warmup + passes
    odom_prev = np.array([10.0, 4.0, 0.1, 0.0, 0.0, 0.34289781, 0.93937271], F)
    odom_cur = odom_prev.copy()
    odom_cur[:3] += np.array([0.001, 0.0005, 0.0], F)        # (a slow robot: the cloud of particles stays on the observation)
    with LocalPlanner([configs.bench_theory("C2")], max_points=1 << 16) as lp:
        pm, poses = setup(lp, n)
        pf = localization.ParticleFilter(lp, localization.shipped_filter_config(
            max_particles=max(n, 64), odom_err_integ_lin_tc=LIN_TC, odom_err_integ_ang_tc=ANG_TC, bias_var_dist=VAR_DIST, bias_var_ang=VAR_ANG))
        s0 = np.zeros((n, 13), F)
        s0[:, :7] = poses
        plan = draws(n, steps, rng)
        pf.set_particles(s0, None, plan[0][2])
        h_states, h_noise, h_prob = s0.copy(), plan[0][2].copy(), np.full(n, F(1.0 / n), F)
        state_prev = s0[0, :7].copy()
        h_prev = state_prev.copy()
        h_est = np.zeros(44, F)
        t_dev, t_host, parts = [], [], {"predict": [], "measure": [], "resample": [], "set_noise": []}
        n_dup = launches = 0
        for i, (u, rows, z) in enumerate(plan):
            a0 = time.perf_counter()
            pf.predict(odom_prev, odom_cur, 0.1)
            a1 = time.perf_counter()
            est = pf.measure(None, None, state_prev)
            a2 = time.perf_counter()
            st = pf.resample(u, rows)
            a3 = time.perf_counter()
            pf.set_noise(z)
            a4 = time.perf_counter()
            state_prev = np.array(est.mean_biased[:], F)
            state_prev[3:7] /= np.linalg.norm(state_prev[3:7])
            b0 = time.perf_counter()
            host.host_predict(n, ptr(h_states), ptr(h_noise), ptr(odom_prev), ptr(odom_cur), 0.1, LIN_TC, ANG_TC)
            like, _ = pm.measure_prepared(np.ascontiguousarray(h_states[:, :7]))
            host.host_update(n, ptr(h_states), ptr(h_noise), ptr(h_prob), ptr(like), ptr(h_prev), VAR_DIST, VAR_ANG, u, ptr(rows), ptr(z),
                             ptr(h_est))
            b1 = time.perf_counter()
            h_prev = h_est[:7].copy()
            h_prev[3:7] /= np.linalg.norm(h_prev[3:7])
            if i >= warmup:
                t_dev.append(a4 - a0)
                t_host.append(b1 - b0)
                for k, v in zip(("predict", "measure", "resample", "set_noise"), (a1 - a0, a2 - a1, a3 - a2, a4 - a3)):
                    parts[k].append(v)
                n_dup += st.n_duplicates
                launches = est.launches + st.launches + 1
    row = {"particles": n, "passes": passes, "device_step": stats_of(t_dev), "host_route_step": stats_of(t_host),
           "device_parts": {k: stats_of(v) for k, v in parts.items()}, "mean_duplicates_per_step": n_dup / passes, "device_launches_per_step": launches}
    row["device_minus_host_us"] = row["device_step"]["median_us"] - row["host_route_step"]["median_us"]
    row["faster"] = "device" if row["device_minus_host_us"] < 0 else "host route"
    print("%5d particles: device step %.1f us (predict %.1f, measure %.1f, resample %.1f, set_noise %.1f), host route %.1f us: %s wins" % (
        n, row["device_step"]["median_us"], *(row["device_parts"][k]["median_us"] for k in ("predict", "measure", "resample", "set_noise")),
        row["host_route_step"]["median_us"], row["faster"]), flush=True)
    return row


def measure_only(particles, passes, warmup):
    from dddmr_navigation_amd import configs
    from dddmr_navigation_amd.local_planner import LocalPlanner
    out = {}
    for n in particles:
        with LocalPlanner([configs.bench_theory("C2")], max_points=1 << 16) as lp:
            pm, poses = setup(lp, n)
            times = []
            for i in range(warmup + passes):
                t0 = time.perf_counter()
                pm.measure_prepared(poses)
                times.append(time.perf_counter() - t0)
        out[str(n)] = stats_of(times[warmup:])
    print(json.dumps({"measure_prepared": out, "library": os.environ.get("DDDMR_LIB_NAME", "shipped")}), flush=True)


def compare_with(name, particles, passes, warmup):
    """mcl_measure_prepared of the shipped library and of csrc/<name> (the parent commit's build), alternating processes"""
    runs = {"parent": [], "shipped": []}
    for _ in range(2):
        for which in ("parent", "shipped"):
            env = dict(os.environ)
            if which == "parent":
                env["DDDMR_LIB_NAME"] = name
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--measure-only", "--passes", str(passes), "--warmup", str(warmup),
                                "--particles", *map(str, particles)], env=env, capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                raise RuntimeError(r.stderr[-2000:])
            runs[which].append(json.loads(r.stdout.strip().split("\n")[-1])["measure_prepared"])
    rows = []
    for n in map(str, particles):
        par, new = [r[n] for r in runs["parent"]], [r[n] for r in runs["shipped"]]
        lo, hi = min(r["p10_us"] for r in par), max(r["p90_us"] for r in par)
        med = statistics.median(r["median_us"] for r in new)
        rows.append({"particles": int(n), "parent_runs": par, "shipped_runs": new, "parent_p10_p90_us": [lo, hi], "shipped_median_us": med,
                     "inside_parent_spread": med <= hi})
        print("measure_prepared at %s particles: parent %.1f - %.1f us (p10 - p90 of two runs), this tree's median %.1f us: %s" % (
            n, lo, hi, med, "inside" if med <= hi else "OUTSIDE"), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, nargs="*", default=[60, 1024, 16384])
    ap.add_argument("--passes", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--measure-only", action="store_true")
    ap.add_argument("--compare-with", help="library name under csrc/ built from the parent commit")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.measure_only:
        return measure_only(args.particles, args.passes, args.warmup)
    report = {"protocol": "host clock around each step (predict, measure, resample, set_noise), median and p10 / p90 of %d steps after %d "
                          "warm-up steps; the device's step and the host route's alternate step by step in one run; the host route is "
                          "mcl_measure_prepared on uploaded states plus tools/mcl_filter_host_step.cpp, the tool's own C++ restatement of the "
                          "host filter (not the reference), both transfers included; random numbers drawn before the clock starts"
                          % (args.passes, args.warmup),
              "observation_points": [100, 550], "steps": [run_steps(n, args.passes, args.warmup) for n in args.particles]}
    if args.compare_with:
        report["measure_prepared_against_parent"] = compare_with(args.compare_with, args.particles, args.passes, args.warmup)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
