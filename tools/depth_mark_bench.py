"""Times dddmr_rollout_depth_mark_clusters on the two-camera scene: observations of about 5000, 10000 and 34000 points,
host clock around the C call (buffers sized once, outside the clock), median and spread of 300 calls, with the
observation grid kept (no depth source published in between) and rebuilt (a frame fed before every call; the feed is
outside the clock).  The NumPy / SciPy restatement's time on the same input stands beside it, labelled as such: it is not
PCL, and no speed-up over the reference follows from it.  Writes profiles/r08_depth_mark.json.

--general times, for the bar of the slice, dddmr_rollout_marking_update on the SAME points handed over as a lidar-fed
observation (set_cloud) with the same tolerance; start it with DDDMR_MARKING_ROUTE=general in the environment.  That
update does this call's work plus clearing, projection and the dGraph.

    python tools/depth_mark_bench.py [--calls 300] [--general] [--out profiles/r08_depth_mark.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

from dddmr_navigation_amd import _capi as K, configs, scenes  # noqa: E402
from dddmr_navigation_amd.local_planner import LocalPlanner  # noqa: E402
import depth_frustum_ref as R  # noqa: E402

OBSERVATIONS = (("obs5k", (112, 84), 1), ("obs10k", (160, 120), 1), ("obs34k", (320, 240), 2))
TOL, RATIO = 0.1, 0.2


def stats(us):
    us = np.sort(np.asarray(us))
    return {"median_us": float(np.median(us)), "p10_us": float(us[len(us) // 10]), "p90_us": float(us[(9 * len(us)) // 10]),
            "min_us": float(us[0]), "max_us": float(us[-1]), "calls": int(len(us))}


def feed(lp, dc, w, h, alive0):
    frames = [scenes.depth_frame(dc.cloud, dc.T_gbl_cam(i), w, h, dc.fov_w, dc.fov_v, dc.d_max, seed=21 + i) for i in range(2)]
    again = scenes.depth_frame(dc.cloud, dc.T_gbl_cam(0), w, h, dc.fov_w, dc.fov_v, dc.d_max, seed=29)
    frs = []
    for i in range(2):
        lp.set_depth_source(i, dc.z_min, dc.z_max, 10**10 if (i == 0 and alive0 == 2) else 0, max_frame_points=w * h,
                            max_frames=2 if i == 0 else 1)
        lp.set_depth_frame(i, frames[i], dc.T_base_cam[i], dc.T_gbl_base, 10**9)
        if i == 0 and alive0 == 2:
            lp.set_depth_frame(0, again, dc.T_base_cam[0], dc.T_gbl_base, 10**9 + 33_000_000)
        lp.set_depth_frustum(i, dc.fov_w, dc.fov_v, dc.d_min, dc.d_max, dc.T_gbl_cam(i))
        frs.append(R.Frustum(dc.fov_w, dc.fov_v, dc.d_min, dc.d_max, dc.T_gbl_cam(i)))
    return frames, frs


def statics(dc):
    gx, gy = np.meshgrid(np.arange(-8.0, 8.001, 0.25), np.arange(-8.0, 8.001, 0.25), indexing="ij")
    t = dc.T_gbl_base
    ground = np.stack([gx.ravel() + t[0], gy.ravel() + t[1], np.full(gx.size, t[2] - 0.05)], axis=1).astype(np.float32)
    return ground, dc.cloud[::40, :3].astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--general", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_depth_mark.json"))
    args = ap.parse_args()
    dc = scenes.depth_clear_scene()
    ground, smap = statics(dc)
    out = {"what": "host clock around one call, microseconds", "cases": []}
    for label, (w, h), alive0 in OBSERVATIONS:
        with LocalPlanner([configs.bench_theory("C2")], max_points=400_000) as lp:
            frames, frs = feed(lp, dc, w, h, alive0)
            obs = lp.get_cloud()
            if args.general:
                from dddmr_navigation_amd import marking
                cfg = marking.shipped_config()
                cfg.euclidean_cluster_extraction_tolerance = TOL
                cfg.segmentation_ignore_ratio = RATIO
                t_bs = (0.0, 0.0, 0.5, 0, 0, 0, 1)
                with LocalPlanner([configs.bench_theory("C2")], max_points=1 << 16) as lq:
                    layer = marking.MarkingLayer(lq, cfg, ground, smap)
                    us = []
                    for k in range(args.calls + 20):
                        lq.set_cloud(obs)
                        t0 = time.perf_counter()
                        st = layer.update(t_bs, dc.T_gbl_base)
                        us.append((time.perf_counter() - t0) * 1e6)
                    routes = layer.route_counts()
                case = {"observation": label, "observation_points": int(len(obs)), "marking_update": stats(us[20:]),
                        "route": os.environ.get("DDDMR_MARKING_ROUTE", "by size"), "routes": routes,
                        "n_clusters": int(st.n_clusters)}
            else:
                import depth_mark_ref as M
                lp.depth_mark_create(dc.res, dc.hres, ground, smap, tolerance=TOL, min_cluster_size=1, segmentation_ignore_ratio=RATIO,
                                     max_observation_points=1 << 16)
                t0 = time.perf_counter()
                ref = M.self_mark(frs, obs[:, :3], ground, smap, dc.res, dc.hres, TOL, 1, RATIO, dc.T_gbl_base)
                numpy_ms = (time.perf_counter() - t0) * 1e3
                got = lp.depth_mark_clusters(dc.T_gbl_base)
                st = got[6]
                same = all(int(getattr(st, k)) == v for k, v in ref["stats"].items())
                c, p = int(st.n_accepted), int(st.n_points)
                bufs = [np.zeros((c + 1, 3), np.float32), np.zeros((c + 1, 3), np.int32), np.zeros(c + 1, np.uint32), np.zeros(c + 1, np.uint32),
                        np.zeros((p + 1, 3), np.float32), np.zeros(4, np.float32)]
                tgb = (C.c_double * 7)(*[float(v) for v in dc.T_gbl_base])
                ptrs = [b.ctypes.data for b in bufs]
                call = lambda: lp._lib.dddmr_rollout_depth_mark_clusters(lp._ctx, tgb, c, p, *ptrs, C.byref(st))
                kept, rebuilt = [], []
                for _ in range(20):
                    assert call() == K.OK
                for _ in range(args.calls):
                    t0 = time.perf_counter()
                    call()
                    kept.append((time.perf_counter() - t0) * 1e6)
                ops_kept = int(st.launches)
                for k in range(args.calls):
                    lp.set_depth_frame(1, frames[1], dc.T_base_cam[1], dc.T_gbl_base, 10**9 + k + 1)
                    t0 = time.perf_counter()
                    call()
                    rebuilt.append((time.perf_counter() - t0) * 1e6)
                case = {"observation": label, "observation_points": int(len(obs)), "n_clusters": int(st.n_clusters), "n_accepted": c,
                        "n_points": p, "counts_equal_to_restatement": bool(same),
                        "grid_kept": dict(stats(kept), device_operations=ops_kept),
                        "grid_rebuilt": dict(stats(rebuilt), device_operations=int(st.launches)),
                        "numpy_scipy_restatement_ms": numpy_ms}
        print(json.dumps(case), flush=True)
        out["cases"].append(case)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
