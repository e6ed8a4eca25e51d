#!/usr/bin/env python3
"""Time of one batch of mcl_3dl measure() calls on the device: dddmr_rollout_mcl_measure for 60, 1024 and 16 384
particles with 100 flat and 550 less-sharp points against a 200 000-point map and a 100 000-point ground.

  python tools/mcl_measure_bench.py --out profiles/r15_mcl_measure.json

Host clock around the call (it ends in its own wait for the device), median and p10 / p90 of --passes calls after
--warmup untimed ones.  No bar is set: nothing earlier does this work, and no CPU figure for the reference is claimed,
because it cannot be built here.  The scene is a 100 m hall: a jittered floor (the ground, also part of the map), walls
and boxes; particles are spread around a true pose as a tracking filter's are, a tenth of them far off.  For the
kernels' own time, in a run of its own:
  rocprofv3 --kernel-trace --stats -- python tools/mcl_measure_bench.py --particles 1024 --passes 50
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import numpy as np  # noqa: E402

N_MAP, N_GROUND, N_FLAT, N_LS = 200_000, 100_000, 100, 550


def hall(rng):
    side = 100.0
    ground = np.concatenate([rng.uniform(-side / 2, side / 2, (N_GROUND, 2)), rng.uniform(-0.02, 0.02, (N_GROUND, 1))], axis=1)
    nrm = np.concatenate([rng.normal(0, 0.05, (N_GROUND, 2)), np.ones((N_GROUND, 1))], axis=1)
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    n_wall = (N_MAP - N_GROUND) // 2
    t = rng.uniform(-side / 2, side / 2, n_wall)
    wall = np.stack([np.where(rng.random(n_wall) < 0.5, -side / 2, side / 2), t, rng.uniform(0, 3, n_wall)], axis=1)
    swap = rng.random(n_wall) < 0.5
    wall[swap, 0], wall[swap, 1] = wall[swap, 1], wall[swap, 0].copy()
    n_box = N_MAP - N_GROUND - n_wall
    centres = rng.uniform(-side / 2 + 2, side / 2 - 2, (200, 2))
    box = np.concatenate([centres[rng.integers(0, 200, n_box)] + rng.uniform(-0.5, 0.5, (n_box, 2)), rng.uniform(0, 1.5, (n_box, 1))], axis=1)
    structure = np.concatenate([wall, box])
    return np.concatenate([ground, structure]).astype(np.float32), ground.astype(np.float32), nrm.astype(np.float32), structure


def scene(n_particles, seed=15):
    import mcl_measure_cases as Cs
    rng = np.random.default_rng(seed)
    static_map, ground, nrm, structure = hall(rng)
    true_pos, yaw = np.array([3.0, -2.0, 0.0]), 0.4
    Rt = Cs.rot_matrix(Cs.quat_rpy(0, 0, yaw))
    g = ground.astype(np.float64)
    near = g[np.linalg.norm(g[:, :2] - true_pos[:2], axis=1) < 8.0]
    flat = (near[rng.choice(len(near), N_FLAT, replace=False)] - true_pos) @ Rt + rng.normal(0, 0.02, (N_FLAT, 3))
    s = structure[np.linalg.norm(structure[:, :2] - true_pos[:2], axis=1) < 30.0]
    ls = (s[rng.choice(len(s), N_LS, replace=False)] - true_pos) @ Rt + rng.normal(0, 0.03, (N_LS, 3))
    ls = np.concatenate([ls, rng.uniform(0.5, 3.0, (N_LS, 1))], axis=1)
    states = np.zeros((n_particles, 7))
    states[:, :3] = true_pos + rng.normal(0, [0.2, 0.2, 0.03], (n_particles, 3))
    far = rng.random(n_particles) < 0.1
    states[far, :2] = rng.uniform(-45, 45, (int(far.sum()), 2))
    for i in range(n_particles):
        states[i, 3:] = Cs.quat_rpy(rng.normal(0, 0.02), rng.normal(0, 0.02), yaw + rng.normal(0, 0.05))
    return static_map, ground, nrm, flat.astype(np.float32), ls.astype(np.float32), states.astype(np.float32)


def measure(n_particles, passes, warmup):
    from dddmr_navigation_amd import configs, localization
    from dddmr_navigation_amd.local_planner import LocalPlanner
    static_map, ground, nrm, flat, ls, states = scene(n_particles)
    with LocalPlanner([configs.bench_theory("C2")], max_points=1 << 16) as lp:
        pm = localization.ParticleMeasure(lp, localization.shipped_config(max_map_points=N_MAP, max_ground_points=N_GROUND,
                                                                           max_particles=max(n_particles, 64)))
        t0 = time.perf_counter()
        pm.set_map(static_map, ground, nrm)
        set_map_ms = 1e3 * (time.perf_counter() - t0)
        times = []
        for i in range(warmup + passes):
            t0 = time.perf_counter()
            like, qual = pm.measure(flat, ls, states)
            t1 = time.perf_counter()
            if i >= warmup:
                times.append(t1 - t0)
        terms = pm.terms(n_particles)
        st = pm.last
    us = sorted(1e6 * t for t in times)
    return {"particles": n_particles, "passes": len(us), "median_us": statistics.median(us), "p10_us": us[len(us) // 10],
            "p90_us": us[(9 * len(us)) // 10], "set_map_ms_once": set_map_ms, "healthy": int(terms["healthy"].sum()),
            "mean_matches": float(terms["n_match"].mean()), "max_ground_neighbours": int(st.max_ground_neighbours_seen),
            "quality_min": float(st.quality_min), "quality_max": float(st.quality_max), "best_likelihood": float(like.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, nargs="*", default=[60, 1024, 16384])
    ap.add_argument("--passes", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out")
    args = ap.parse_args()
    report = {"protocol": "host clock around dddmr_rollout_mcl_measure (upload, three kernels, the wait for the result word), median and "
                          "p10 / p90 of %d calls after %d warm-up calls; %d flat + %d less-sharp points, %d map points, %d ground points; "
                          "no CPU figure for the reference: it cannot be built here" % (args.passes, args.warmup, N_FLAT, N_LS, N_MAP, N_GROUND),
              "sizes": []}
    for n in args.particles:
        r = measure(n, args.passes, args.warmup)
        report["sizes"].append(r)
        print("%6d particles: %.1f us (p10 %.1f, p90 %.1f), %d on trusted ground, %.1f matches per particle" % (
            n, r["median_us"], r["p10_us"], r["p90_us"], r["healthy"], r["mean_matches"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
