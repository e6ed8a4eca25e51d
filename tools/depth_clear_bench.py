"""Times dddmr_rollout_depth_clear_verdicts on the two-camera scene: 2000 / 8000 markings of the scene's cluster sizes
against an observation of about 5000 and about 40000 points, host clock around the call, median and spread of 300 calls,
with the grid kept (no depth source published in between) and rebuilt (a frame fed before every call; the feed is outside
the clock).  The NumPy restatement's time on the same inputs stands beside it, labelled as NumPy: it is not PCL, and no
speed-up over the reference follows from it.  Writes profiles/r06_depth_clear.json.

    python tools/depth_clear_bench.py [--calls 300] [--out profiles/r06_depth_clear.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

from dddmr_navigation_amd import configs, scenes  # noqa: E402
from dddmr_navigation_amd.local_planner import LocalPlanner  # noqa: E402
import depth_frustum_ref as R  # noqa: E402


def stats(us):
    us = np.sort(np.asarray(us))
    return {"median_us": float(np.median(us)), "p10_us": float(us[len(us) // 10]), "p90_us": float(us[(9 * len(us)) // 10]),
            "min_us": float(us[0]), "max_us": float(us[-1]), "calls": int(len(us))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r06_depth_clear.json"))
    args = ap.parse_args()
    dc = scenes.depth_clear_scene()
    out = {"what": "host clock around dddmr_rollout_depth_clear_verdicts, microseconds", "cases": []}
    # obs40k: the left camera keeps two frames alive (observation_persistence > 0), the right one its newest
    for label, (w, h), alive0 in (("obs5k", (112, 84), 1), ("obs40k", (320, 240), 2)):
        frames = [scenes.depth_frame(dc.cloud, dc.T_gbl_cam(i), w, h, dc.fov_w, dc.fov_v, dc.d_max, seed=21 + i) for i in range(2)]
        again = scenes.depth_frame(dc.cloud, dc.T_gbl_cam(0), w, h, dc.fov_w, dc.fov_v, dc.d_max, seed=29)
        with LocalPlanner([configs.bench_theory("C2")], max_points=400_000) as lp:
            frs = []
            for i in range(2):
                lp.set_depth_source(i, dc.z_min, dc.z_max, 10**10 if (i == 0 and alive0 == 2) else 0, max_frame_points=w * h,
                                    max_frames=2 if i == 0 else 1)
                lp.set_depth_frame(i, frames[i], dc.T_base_cam[i], dc.T_gbl_base, 10**9)
                if i == 0 and alive0 == 2:
                    lp.set_depth_frame(0, again, dc.T_base_cam[0], dc.T_gbl_base, 10**9 + 33_000_000)
                lp.set_depth_frustum(i, dc.fov_w, dc.fov_v, dc.d_min, dc.d_max, dc.T_gbl_cam(i))
                frs.append(R.Frustum(dc.fov_w, dc.fov_v, dc.d_min, dc.d_max, dc.T_gbl_cam(i)))
            obs = lp.get_cloud()[:, :3]
            for m in (2000, 8000):
                vox, off, cl = dc.markings(obs, n=m, seed=5)
                t0 = time.perf_counter()
                want_v, want_e, ok = R.clear_verdicts(frs, obs, dc.res, dc.hres, vox, off, cl)
                numpy_ms = (time.perf_counter() - t0) * 1e3
                got_v, got_e = lp.depth_clear_verdicts(dc.res, dc.hres, vox, off, cl)
                same = bool(np.array_equal(got_v[ok], want_v[ok]) and np.array_equal(got_e[ok], want_e[ok]))
                kept, rebuilt = [], []
                for _ in range(20):
                    lp.depth_clear_verdicts(dc.res, dc.hres, vox, off, cl)
                for _ in range(args.calls):
                    t0 = time.perf_counter()
                    lp.depth_clear_verdicts(dc.res, dc.hres, vox, off, cl)
                    kept.append((time.perf_counter() - t0) * 1e6)
                launches_kept = lp.depth_clear_launches()
                for k in range(args.calls):
                    lp.set_depth_frame(1, frames[1], dc.T_base_cam[1], dc.T_gbl_base, 10**9 + k + 1)
                    t0 = time.perf_counter()
                    lp.depth_clear_verdicts(dc.res, dc.hres, vox, off, cl)
                    rebuilt.append((time.perf_counter() - t0) * 1e6)
                case = {"observation": label, "observation_points": int(len(obs)), "markings": int(m), "cluster_points": int(off[-1]),
                        "equal_to_restatement_where_margins_hold": same, "compared": int(ok.sum()),
                        "grid_kept": dict(stats(kept), device_operations=launches_kept),
                        "grid_rebuilt": dict(stats(rebuilt), device_operations=lp.depth_clear_launches()),
                        "numpy_restatement_ms": numpy_ms}
                print(json.dumps(case))
                out["cases"].append(case)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
