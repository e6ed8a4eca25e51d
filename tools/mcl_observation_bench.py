#!/usr/bin/env python3
"""Time of the localiser's observation on the device: dddmr_rollout_mcl_prepare, dddmr_rollout_mcl_prepare_from_sweep and
dddmr_rollout_mcl_measure_prepared, and -- in the same run, alternating call by call -- dddmr_rollout_mcl_measure on the
arrays dddmr_rollout_mcl_get_observation returned (the unchanged path: the baseline of measure_prepared).

  python tools/mcl_observation_bench.py --out profiles/r17_mcl_observation.json

Host clock around each call (each ends in its own wait for the device), median and p10 / p90 of --passes calls after
--warmup untimed ones.  Inputs: 100 flat / 550 less-sharp points (what the shipped configuration sees) and 384 / 1616
(384 is a 16-ring sweep's flat maximum; its less-sharp maximum of 1920 does not fit beside it under the library's 2000
observation points), each with 60 and 1024 particles in mcl_measure_bench's hall.  prepare_from_sweep runs on the
features of the 16 x 1000 test sweep.  The only bar: measure_prepared is not slower than mcl_measure on the same
observation by more than the run's own spread (p90 - p10 of mcl_measure).  No CPU figure for the host function is
claimed: it needs PCL, which cannot be built here.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

SIZES = ((100, 550), (384, 1616))


def stats_of(times):
    us = sorted(1e6 * t for t in times)
    return {"median_us": statistics.median(us), "p10_us": us[len(us) // 10], "p90_us": us[(9 * len(us)) // 10]}


def timed(fn, n):
    out = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out


def run_size(n_flat, n_ls, particles, passes, warmup):
    import mcl_measure_bench as mb
    import mcl_observation_cases as oc
    from dddmr_navigation_amd import configs, localization
    from dddmr_navigation_amd.local_planner import LocalPlanner
    mb.N_FLAT, mb.N_LS = n_flat, n_ls
    rows = []
    with LocalPlanner([configs.bench_theory("C2")], max_points=1 << 16) as lp:
        pm = localization.ParticleMeasure(lp, localization.shipped_config(max_map_points=mb.N_MAP, max_ground_points=mb.N_GROUND,
                                                                           max_particles=max(max(particles), 64)))
        pm.configure_observation(localization.shipped_observation_config(max_flat_points=n_flat, max_less_sharp_points=n_ls))
        have_map = False
        for n in particles:
            static_map, ground, nrm, flat, ls, states = mb.scene(n)
            if not have_map:
                pm.set_map(static_map, ground, nrm)
                have_map = True
            flat_s, ls_s = oc.to_sensor(flat), oc.to_sensor(ls[:, :3])
            t_prepare = timed(lambda: pm.prepare(flat_s, ls_s, oc.T_B2S), warmup + passes)[warmup:]
            st = pm.last_observation
            f, l, _ = pm.observation()
            t_prepared, t_measure = [], []
            for i in range(warmup + passes):                    # alternating: the same device state, the same clocks
                a = timed(lambda: pm.measure_prepared(states), 1)[0]
                b = timed(lambda: pm.measure(f, l, states), 1)[0]
                if i >= warmup:
                    t_prepared.append(a)
                    t_measure.append(b)
            like_a, _ = pm.measure_prepared(states)
            like_b, _ = pm.measure(f, l, states)
            assert like_a.tobytes() == like_b.tobytes()
            row = {"n_flat_in": n_flat, "n_less_sharp_in": n_ls, "particles": n, "passes": passes, "branch": int(st.branch),
                   "n_flat_out": int(st.n_flat_out), "n_less_sharp_out": int(st.n_less_sharp_out), "n_clusters": int(st.n_clusters),
                   "launches": int(st.launches), "host_waits": int(st.host_waits), "prepare": stats_of(t_prepare),
                   "measure_prepared": stats_of(t_prepared), "mcl_measure_same_arrays": stats_of(t_measure)}
            m = row["mcl_measure_same_arrays"]
            row["spread_us"] = m["p90_us"] - m["p10_us"]
            row["prepared_minus_measure_us"] = row["measure_prepared"]["median_us"] - m["median_us"]
            row["bar_met"] = row["prepared_minus_measure_us"] <= row["spread_us"]
            rows.append(row)
            print("%4d / %4d points, %5d particles: prepare %.1f us (branch %d, %d launches), measure_prepared %.1f us, mcl_measure %.1f us "
                  "(spread %.1f us): %s" % (n_flat, n_ls, n, row["prepare"]["median_us"], st.branch, st.launches,
                                            row["measure_prepared"]["median_us"], m["median_us"], row["spread_us"],
                                            "bar met" if row["bar_met"] else "BAR MISSED"), flush=True)
    return rows


def run_sweep(passes, warmup):
    import lidar_features_cases as FC
    import mcl_observation_cases as oc
    from dddmr_navigation_amd import configs, localization, scenes
    from dddmr_navigation_amd.local_planner import LocalPlanner
    c, raw, _, _ = FC.case("16x1000-g7-m0.0")
    tbs = (0.1, 0.0, 0.6) + tuple(scenes.quat_from_rpy(0.0, 0.0, 0.05))
    tgb = (1.0, -0.5, 0.0) + tuple(scenes.quat_from_rpy(0.0, 0.0, 0.3))
    with LocalPlanner([configs.bench_theory("C2")], max_points=200_000) as lp:
        args, kwargs = c.planner_args()
        lp.set_lidar_sweep_source(0, *args, **kwargs)
        lp.set_lidar_sweep_features(0, FC.EDGE, FC.SURF)
        lp.set_lidar_sweep(0, raw, tbs, tgb, 8.0, 1.8)
        flat, ls = lp.get_lidar_sweep_features(0, 2)[0], lp.get_lidar_sweep_features(0, 1)[0]
        pm = localization.ParticleMeasure(lp, localization.shipped_config(max_map_points=1024, max_ground_points=1024, max_particles=64))
        pm.configure_observation(localization.shipped_observation_config())
        t_sweep = timed(lambda: pm.prepare_from_sweep(0, oc.T_B2S), warmup + passes)[warmup:]
        st = pm.last_observation
        t_host = timed(lambda: pm.prepare(flat, ls, oc.T_B2S), warmup + passes)[warmup:]
    row = {"sweep": "16x1000-g7-m0.0", "n_flat_in": len(flat), "n_less_sharp_in": len(ls), "branch": int(st.branch), "launches": int(st.launches),
           "prepare_from_sweep": stats_of(t_sweep), "prepare_same_lists_from_the_host": stats_of(t_host)}
    print("sweep 16 x 1000 (%d / %d points): prepare_from_sweep %.1f us, prepare from host arrays %.1f us" % (
        len(flat), len(ls), row["prepare_from_sweep"]["median_us"], row["prepare_same_lists_from_the_host"]["median_us"]), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, nargs="*", default=[60, 1024])
    ap.add_argument("--passes", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out")
    args = ap.parse_args()
    report = {"protocol": "host clock around each call, median and p10 / p90 of %d calls after %d warm-up calls; measure_prepared and "
                          "mcl_measure (on the arrays get_observation returned) alternate call by call in one run; spread = p90 - p10 of "
                          "mcl_measure; bar: median(measure_prepared) - median(mcl_measure) <= spread; no CPU figure for "
                          "cbLeGoFeatureCloud: it cannot be built here" % (args.passes, args.warmup),
              "sizes": [], "sweep": None}
    for n_flat, n_ls in SIZES:
        report["sizes"] += run_size(n_flat, n_ls, args.particles, args.passes, args.warmup)
    report["sweep"] = run_sweep(args.passes, args.warmup)
    report["bar_met"] = all(r["bar_met"] for r in report["sizes"])
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
