#!/usr/bin/env python3
"""Per-frame time of the depth camera feed (dddmr_rollout_set_depth_frame) on the GPU, against the only device path
such a frame had before it: dddmr_rollout_set_scan_source fed the same raw frame (window wide open).

  python tools/depth_feed_bench.py --baseline-lib PATH --out profiles/r04_depth_feed.json

Every measurement runs in a child process of its own (a fresh context; the baseline library is loaded with plain
ctypes, it need not export the depth entry points).  The two libraries alternate, --rounds times; a figure is the
median over --frames timed calls after --warmup untimed ones, host clock around the call (which ends in the feed's own
wait for the device).  `--worker` is the child's entry; `--profile-worker` runs a short loop for a kernel trace
(rocprofv3 --kernel-trace --stats -- python tools/depth_feed_bench.py --profile-worker ...).

  python tools/depth_feed_bench.py --image --baseline-lib PATH [--variant-lib NAME=PATH ...] --out profiles/r05_depth_image.json

measures the depth image path (dddmr_rollout_set_depth_image, the uint16 image of the view at sample_step 1) against the
parent commit's dddmr_rollout_set_depth_frame fed the driver's organised cloud of the same view (every pixel, 16-byte
records), same protocol.  Reported beside it without a bar: sample_step 2 and 4, the parent's set_depth_frame fed the
stage-one cloud prepared on the host (with the host time of this tool's NumPy stage one, which is not PCL's), and any
--variant-lib builds (such as one pixel per lane) at sample_step 1.
"""
import argparse
import ctypes as C
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

TBS = (0.2, 0.0, 0.3, 0.0, 0.024997395914712332, 0.0, 0.9996875162757026)   # camera mount, 0.05 rad nose-down
TGB = (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0)
SHAPES = {"640x480": (640, 480), "848x480": (848, 480)}


def make_frame(shape, branch):
    """branch 'voxel': the C2 scene as rendered (> 20000 survivors); 'pass': the same frame thinned to 20000 survivors"""
    from dddmr_navigation_amd import scenes
    import depth_feed_ref as R
    w, h = SHAPES[shape]
    fr = scenes.depth_frame(scenes.cloud_c2(), R.compose(TGB, TBS), w, h, 1.5, 1.0, 8.0, seed=9)
    if branch == "pass":
        base = R.transform(np.nan_to_num(fr, nan=0.0), TBS)
        z = base[:, 2].astype(np.float64)
        alive = np.flatnonzero(np.isfinite(fr).all(axis=1) & (z >= 0.0) & (z <= 2.0))
        fr[alive[20000:]] = np.nan
    return fr, R.n_survivors(fr, TBS, 0.0, 2.0)


IMAGE_NODE = dict(max_distance=6.0, leaf_size=0.05)      # the shipped launch's; sample_step is the case's


def make_image(shape):
    from dddmr_navigation_amd import scenes
    import depth_feed_ref as R
    w, h = SHAPES[shape]
    img, k4 = scenes.depth_image(scenes.cloud_c2(), R.compose(TGB, TBS), w, h, 1.5, 1.0, 8.0, seed=9)
    return img, k4, R.compose(TBS, scenes.T_LINK_OPTICAL)


def worker(args):
    from dddmr_navigation_amd import _capi as K, configs
    lib = C.CDLL(args.lib)
    host_stage_one_ms = None
    if args.path == "image":
        img, k4, tbo = make_image(args.shape)
        fr, surv = img, 0
        n = -(-img.shape[0] // args.step) * -(-img.shape[1] // args.step)
    elif args.path == "stage1cloud":
        import depth_image_ref as I
        img, k4, tbo = make_image(args.shape)
        t0 = time.perf_counter()
        fr = np.ascontiguousarray(I.stage_one(img, k4, sample_step=args.step, **IMAGE_NODE))
        host_stage_one_ms = (time.perf_counter() - t0) * 1e3
        surv = len(fr)
        n = len(fr)
    else:
        fr, surv = make_frame(args.shape, args.branch)
        if args.stride == 16:
            fr = np.ascontiguousarray(np.concatenate([fr, np.ones((len(fr), 1), np.float32)], axis=1))
        n = len(fr)
    theories = configs.theory_array([configs.bench_theory("C2")])
    cfg = K.RolloutConfig()
    cfg.abi_version, cfg.device, cfg.rank, cfg.world_size = K.ABI_VERSION, 0, 0, 1
    cfg.max_points, cfg.max_trajectories, cfg.max_steps, cfg.max_plan_poses = max(n, 1 << 19), 65536, 256, 256
    cfg.n_theories = len(theories)
    cfg.theories = C.cast(theories, C.POINTER(K.TheoryConfig))
    ctx = C.c_void_p()
    lib.dddmr_rollout_create.argtypes = [C.POINTER(K.RolloutConfig), C.POINTER(C.c_void_p)]
    lib.dddmr_rollout_destroy.argtypes = [C.c_void_p]
    lib.dddmr_rollout_destroy.restype = None
    if lib.dddmr_rollout_create(C.byref(cfg), C.byref(ctx)) != 0:
        raise SystemExit("dddmr_rollout_create failed: a HIP device is required")
    tbs, tgb = (C.c_double * 7)(*TBS), (C.c_double * 7)(*TGB)
    n_a, n_b, n_c = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    ptr = fr.ctypes.data_as(C.c_void_p)
    if args.path == "image":
        tbo_c = (C.c_double * 7)(*tbo)
        n_d = C.c_uint32(0)
        lib.dddmr_rollout_set_depth_image_source.argtypes = [C.c_void_p, C.c_int32, C.POINTER(K.DepthSourceConfig), C.POINTER(K.DepthImageConfig)]
        lib.dddmr_rollout_set_depth_image.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t, C.POINTER(C.c_double),
                                                      C.POINTER(C.c_double), C.c_int64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                                      C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        dcfg = K.DepthSourceConfig(0.0, 2.0, 0, n, 1)
        icfg = K.DepthImageConfig(img.shape[1], img.shape[0], *k4, IMAGE_NODE["max_distance"], IMAGE_NODE["leaf_size"], args.step, 0)
        assert lib.dddmr_rollout_set_depth_image_source(ctx, 1, C.byref(dcfg), C.byref(icfg)) == 0
        stamp = [10**9]

        def call():
            stamp[0] += 33_333_333
            return lib.dddmr_rollout_set_depth_image(ctx, 1, ptr, img.strides[0], tbo_c, tgb, stamp[0], C.byref(n_d), C.byref(n_a),
                                                     C.byref(n_b), C.byref(n_c))
    elif args.path in ("depth", "stage1cloud"):
        if args.path == "stage1cloud":
            tbs = (C.c_double * 7)(*tbo)
        rec = fr.strides[0]
        lib.dddmr_rollout_set_depth_source.argtypes = [C.c_void_p, C.c_int32, C.POINTER(K.DepthSourceConfig)]
        lib.dddmr_rollout_set_depth_frame.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_double),
                                                      C.POINTER(C.c_double), C.c_int64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                                      C.POINTER(C.c_uint32)]
        dcfg = K.DepthSourceConfig(0.0, 2.0, 0, n, 1)
        assert lib.dddmr_rollout_set_depth_source(ctx, 1, C.byref(dcfg)) == 0
        stamp = [10**9]

        def call():
            stamp[0] += 33_333_333
            return lib.dddmr_rollout_set_depth_frame(ctx, 1, ptr, n, rec, tbs, tgb, stamp[0], C.byref(n_a), C.byref(n_b), C.byref(n_c))
    else:
        lib.dddmr_rollout_set_scan_source.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_double),
                                                      C.POINTER(C.c_double), C.c_double, C.c_double, C.POINTER(C.c_uint32),
                                                      C.POINTER(C.c_uint32)]

        def call():
            return lib.dddmr_rollout_set_scan_source(ctx, 1, ptr, n, 12, tbs, tgb, 1000.0, 2.0, C.byref(n_a), C.byref(n_c))
    for _ in range(args.warmup):
        assert call() == 0
    times = []
    for _ in range(args.frames):
        t0 = time.perf_counter_ns()
        rc = call()
        times.append(time.perf_counter_ns() - t0)
        assert rc == 0
    lib.dddmr_rollout_destroy(ctx)
    if args.profile_worker:
        return
    times_us = np.asarray(times) / 1e3
    print("RESULT " + json.dumps({"path": args.path, "shape": args.shape, "branch": args.branch, "raw_points": n, "survivors": surv,
                                  "step": args.step, "bytes_per_call": int(fr.nbytes) if args.path != "image" else int(-(-fr.shape[0] // args.step) * fr.shape[1] * 2),
                                  "host_stage_one_numpy_ms": host_stage_one_ms,
                                  "points_out": int(n_a.value), "frames": args.frames, "median_us": float(np.median(times_us)),
                                  "p10_us": float(np.percentile(times_us, 10)), "p90_us": float(np.percentile(times_us, 90))}))


def run_child(lib, path, shape, branch, args, step=1, stride=12):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--lib", lib, "--path", path, "--shape", shape, "--branch", branch,
           "--frames", str(args.frames), "--warmup", str(args.warmup), "--step", str(step), "--stride", str(stride)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.child_timeout)
    if r.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)} failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")     # nothing more runs on the GPU
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def image_main(args):
    variants = dict(v.split("=", 1) for v in args.variant_lib)
    cases = []
    for shape in sorted(SHAPES):
        new, base = [], []
        for _ in range(args.rounds):                          # alternate the two builds
            base.append(run_child(args.baseline_lib, "depth", shape, "voxel", args, stride=16))
            new.append(run_child(args.lib, "image", shape, "voxel", args, step=1))
        bm = [r["median_us"] for r in base]
        nm = [r["median_us"] for r in new]
        case = {"shape": shape, "pixels": base[0]["raw_points"],
                "set_depth_image_step1_median_us": statistics.median(nm), "set_depth_image_step1_rounds_us": nm,
                "image_bytes_per_call": new[0]["bytes_per_call"], "image_points_out": new[0]["points_out"],
                "parent_set_depth_frame_organised_median_us": statistics.median(bm), "parent_set_depth_frame_organised_rounds_us": bm,
                "parent_spread_us": max(bm) - min(bm), "organised_bytes_per_call": base[0]["bytes_per_call"],
                "organised_points_out": base[0]["points_out"]}
        case["accepted"] = case["set_depth_image_step1_median_us"] < case["parent_set_depth_frame_organised_median_us"] - case["parent_spread_us"]
        for step in (2, 4):                                   # reported, no bar
            r = run_child(args.lib, "image", shape, "voxel", args, step=step)
            case["set_depth_image_step%d_median_us" % step] = r["median_us"]
            h = run_child(args.baseline_lib, "stage1cloud", shape, "voxel", args, step=step)
            case["parent_set_depth_frame_host_stage_one_cloud_step%d" % step] = {
                "median_us": h["median_us"], "points_in": h["raw_points"], "bytes_per_call": h["bytes_per_call"],
                "host_stage_one_numpy_ms": h["host_stage_one_numpy_ms"]}
        for name, path in variants.items():
            case["variant_%s_step1_median_us" % name] = run_child(path, "image", shape, "voxel", args, step=1)["median_us"]
        print(json.dumps(case), flush=True)
        cases.append(case)
    out = {"what": "host clock around one call, median of %d calls after %d warm-up calls, %d alternations of the two builds"
                   % (args.frames, args.warmup, args.rounds),
           "yardstick": "parent commit's dddmr_rollout_set_depth_frame fed the organised cloud of the same view (every pixel, 16-byte "
                        "records); the new call gets the uint16 image of that view at sample_step 1, max_distance 6.0, leaf 0.05",
           "bar": "new median below the parent's median by more than the parent's spread (max - min of its rounds)",
           "cases": cases}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    print("ACCEPTED" if all(c["accepted"] for c in cases) else "NOT ACCEPTED")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--profile-worker", action="store_true")
    ap.add_argument("--lib", default=os.path.join(ROOT, "dddmr_navigation_amd", "csrc", "libdddmr_rollout.so"))
    ap.add_argument("--baseline-lib", help="libdddmr_rollout.so built from the parent commit")
    ap.add_argument("--path", choices=["depth", "scan", "image", "stage1cloud"], default="depth")
    ap.add_argument("--image", action="store_true", help="measure the depth image path (see the module's docstring)")
    ap.add_argument("--variant-lib", action="append", default=[], metavar="NAME=PATH", help="--image: further builds, sample_step 1")
    ap.add_argument("--step", type=int, default=1)
    ap.add_argument("--stride", type=int, choices=[12, 16], default=12)
    ap.add_argument("--shape", choices=sorted(SHAPES), default="640x480")
    ap.add_argument("--branch", choices=["voxel", "pass"], default="voxel")
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--child-timeout", type=int, default=120)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.worker or args.profile_worker:
        return worker(args)
    if not args.baseline_lib:
        raise SystemExit("--baseline-lib is required: the yardstick is the parent commit's library")
    if args.image:
        return image_main(args)
    cases = []
    for shape in sorted(SHAPES):
        for branch in ("voxel", "pass"):
            new, base = [], []
            for _ in range(args.rounds):                      # alternate the two builds
                base.append(run_child(args.baseline_lib, "scan", shape, branch, args))
                new.append(run_child(args.lib, "depth", shape, branch, args))
            bm = [r["median_us"] for r in base]
            nm = [r["median_us"] for r in new]
            case = {"shape": shape, "branch": branch, "raw_points": new[0]["raw_points"], "survivors": new[0]["survivors"],
                    "depth_points_out": new[0]["points_out"], "scan_points_out": base[0]["points_out"],
                    "set_depth_frame_median_us": statistics.median(nm), "set_depth_frame_rounds_us": nm,
                    "parent_set_scan_source_median_us": statistics.median(bm), "parent_set_scan_source_rounds_us": bm,
                    "parent_spread_us": max(bm) - min(bm),
                    "raw_bytes_per_frame": new[0]["raw_points"] * 12}
            case["accepted"] = case["set_depth_frame_median_us"] <= case["parent_set_scan_source_median_us"] + case["parent_spread_us"]
            print(json.dumps(case), flush=True)
            cases.append(case)
    out = {"what": "host clock around one call, median of %d calls after %d warm-up calls, %d alternations of the two builds"
                   % (args.frames, args.warmup, args.rounds),
           "yardstick": "parent commit's dddmr_rollout_set_scan_source on the same raw frame, window 1000 m, height 2 m (leaf 0.1 m)",
           "cases": cases}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    ok = all(c["accepted"] for c in cases if c["branch"] == "voxel")
    print("ACCEPTED" if ok else "NOT ACCEPTED")


if __name__ == "__main__":
    main()
