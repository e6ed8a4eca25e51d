#!/usr/bin/env python3
"""What the Python binding hands to the C library, call by call, without a library or a GPU.

A LocalPlanner is made without __init__, its `_lib` is a stand-in whose functions note their name and arguments and
return OK, and a fixed script calls every public method of LocalPlanner, MarkingLayer, DepthLayer, PerceptionStack and
ParticleMeasure once on tiny inputs, then the cloud-taking ones once more on empty inputs.  tests/test_binding_trace_cpu.py
replays the script on the tree and compares with tests/golden/binding_trace.json, which was recorded from the package
as it was before the binding moved to one signature table and shared marshalling helpers:

    git archive <that commit> | tar -x -C /tmp/before
    python tools/binding_trace.py --package-root /tmp/before --out tests/golden/binding_trace.json

What is noted per argument (include/dddmr_rollout.h decides which it is): a number as it is, a double as hex, a string
as text, a pointer to const as the hex bytes behind it, any other pointer as "out", a null pointer as "null".  The
stand-in writes 2 into every size_t count and into the stats fields that size a second call, so two-call getters go on.
"""
import argparse
import ctypes as C
import json
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import capi_header  # noqa: E402

# Inputs that a caller may pass as a plain address: argument index (the context is 0) -> bytes behind it, from the
# call's other arguments.
_ADDRESSED = {
    "depth_frustum_test": {1: lambda a: a[2] * a[3]},
    "depth_clear_verdicts": {3: lambda a: a[6] * 12, 4: lambda a: (a[6] + 1) * 4,
                             5: lambda a: 12 * struct.unpack("<I", C.string_at(_address(a[4]) + a[6] * 4, 4))[0]},
    "depth_mark_create": {2: lambda a: a[3] * a[4], 5: lambda a: a[6] * a[7]},
    "depth_layer_create": {2: lambda a: a[3] * a[4], 5: lambda a: a[6] * a[7]},
    "selftest_sincos": {1: lambda a: a[2] * 8},
}
_SIZING_STATS = ("n_accepted", "n_points", "n_less_sharp_in")


def _address(v):
    return v if isinstance(v, int) else C.cast(v, C.c_void_p).value


def _value(v):
    return v.value if hasattr(v, "value") else v


class Recorder:
    """Stands in for the loaded library: any dddmr_rollout_* attribute is a function that notes its call."""

    def __init__(self):
        self.calls = []
        self._kinds = capi_header.prototypes()

    def __getattr__(self, name):
        if not name.startswith("dddmr_rollout_"):
            raise AttributeError(name)
        ret, kinds = self._kinds[name]
        short = name[len("dddmr_rollout_"):]

        def fn(*args):
            assert len(args) == len(kinds), (name, len(args), len(kinds))
            self.calls.append([short] + [self._note(short, i, k, args) for i, k in enumerate(kinds)])
            return None if ret == "void" else 0
        return fn

    def _note(self, short, i, kind, args):
        v = args[i]
        if kind == "double":
            return float(_value(v)).hex()
        if kind not in ("in", "out"):
            return int(_value(v))
        if v is None or (isinstance(v, C.c_void_p) and v.value is None):
            return "null"
        obj = getattr(v, "_obj", None)                       # byref(x)
        if kind == "out":
            if isinstance(obj, C.c_size_t):
                obj.value = 2
            for f in _SIZING_STATS:
                if hasattr(obj, f):
                    setattr(obj, f, 2)
            return "out"
        if isinstance(v, bytes):
            return v.decode()
        if obj is not None:
            return bytes(obj).hex()
        if isinstance(v, C.Array):
            return bytes(v).hex()
        if hasattr(v, "_arr"):                               # numpy's data_as keeps the array
            return v._arr.tobytes().hex()
        n = _ADDRESSED[short][i]([_value(a) if not isinstance(a, (bytes, C.Array)) and a is not None else a for a in args])
        return C.string_at(_address(v), n).hex()


def record():
    """Run the script on the importable dddmr_navigation_amd -> the list of noted calls."""
    import numpy as np
    from dddmr_navigation_amd import _capi as K, depth_layer, localization, marking, stack
    from dddmr_navigation_amd.local_planner import LocalPlanner, Trajectory

    rec = Recorder()
    lp = object.__new__(LocalPlanner)
    lp._lib, lp._ctx, lp.last_result = rec, C.c_void_p(), None       # (a null handle: close() then calls nothing)

    f32 = lambda rows, cols, start=0.5: (np.arange(rows * cols, dtype=np.float64).reshape(rows, cols) * 0.25 + start).astype(np.float32)
    T1, T2 = (0.1, 0.2, 0.3, 0.0, 0.0, 0.6, 0.8), (1.0, -2.0, 0.5, 0.0, 0.0, 0.0, 1.0)
    T34 = np.arange(12, dtype=np.float64).reshape(3, 4) * 0.5
    tick_in = K.TickInput((C.c_double * 7)(*T2), (C.c_double * 3)(0.5, 0.0, 0.1), 1.0, 0.25)
    img = (np.arange(12, dtype=np.uint16) * 100).reshape(3, 4)

    def feed(cloud3, cloud4, cloud6_f64):
        lp.set_cloud(cloud4)
        lp.set_cloud(cloud6_f64)
        lp.set_scan(cloud3, T1, T2, 5.0, 2.0)
        lp.set_scan_source(1, cloud4, T1, T2, 5.0, 2.0)
        lp.set_depth_frame(2, cloud3, T1, T2, 123456789)
        lp.set_lidar_sweep(0, cloud4, T1, T2, 8.0, 2.0)
        lp.depth_frustum_test(cloud3)

    # -- LocalPlanner ------------------------------------------------------------------------------------------------
    feed(f32(5, 3), f32(4, 4), np.arange(18, dtype=np.float64).reshape(3, 6))
    lp.set_stitcher(3)
    lp.set_stitcher_source(1, 2)
    lp.set_depth_source(2, 0.0, 2.0, 5, max_frame_points=64, max_frames=2)
    lp.set_depth_image_source(3, 0.0, 2.0, 4, 3, 2.0, 2.0, 1.5, 1.0, sample_step=1, drop_zero=True)
    lp.set_depth_image(3, img, T1, T2, 42)
    lp.set_depth_image(3, np.asfortranarray(img), T1, T2, 43)
    lp.get_depth_image_cloud(3)
    lp.set_lidar_sweep_source(0, 16, 64, -15.0, 15.0, 7)
    lp.get_lidar_sweep_cloud(0)
    lp.get_lidar_sweep_image(0, 2, 3)
    lp.set_lidar_sweep_features(0, 0.1, 0.2, T_out=T34)
    lp.set_lidar_sweep_features(0)
    lp.set_lidar_sweep_features(0, enable=False)
    lp.get_lidar_sweep_segmented(0, 4)
    lp.get_lidar_sweep_features(0, 1)
    lp.set_depth_frustum(2, 1.2, 0.9, 0.3, 4.0, T1)
    lp.get_depth_frustum(2)
    lp.depth_clear_verdicts(0.05, 0.1, np.arange(6).reshape(2, 3), [0, 1, 3], f32(3, 3))
    lp.depth_clear_launches()
    lp.depth_mark_create(0.05, 0.1, f32(4, 3), f32(3, 4), tolerance=0.2, min_cluster_size=2)
    lp.depth_mark_clusters(T2)
    lp.get_cloud()
    lp.setPlan(np.arange(14, dtype=np.float64).reshape(2, 7))
    lp.path_blocked(f32(3, 4), 0.5)
    lp.samples("differential_drive_simple", tick_in)
    lp.tick("differential_drive_simple", tick_in)
    lp.tick_begin("differential_drive_simple", tick_in)
    lp.tick_end()
    lp.computeVelocityCommand("differential_drive_simple", Trajectory(), tick_in)
    lp.resolve(12345)
    lp.winner_words()
    lp.resolve_words([1, -2, 3, -4])
    lp.comm_unique_id()
    lp.comm_init(bytes(range(128)), 1, 2)
    lp.comm_ranks()
    lp.comm_loopback()
    lp.comm_loopback_set_peer(1, (7, -8))
    lp.comm_destroy()
    lp.stream_ceiling(1 << 20, 3)
    lp.selftest_sincos([0.0, 0.5, 1.0])
    lp.selftest_wave_ops([1, 2, 0xFFFFFFFF], [1, 0, 1], 5)
    lp.selftest_wave_wide([3, 0xFFFFFFFE], np.arange(64), 2)
    lp.selftest_point_grid(f32(2, 3), (0.0, 0.0, 0.0), (2.0, 2.0, 1.0), 0.25, 0.5, 4096, f32(1, 3, 1.0), 0.1001, 0.01, 2)
    lp.debug()
    lp.pose_arrays()
    lp.pose_arrays(accepted_only=True)
    lp.heading_rows()
    lp.fused_walk()
    lp.best_poses()
    lp.best_cuboids()

    # -- the layers, the stack, the particle measure -------------------------------------------------------------------
    ml = marking.MarkingLayer(lp, marking.shipped_config(max_markings=64), f32(5, 3), f32(3, 4))
    ml.update(T1, T2)
    ml.route_counts(), ml.points(), ml.points(with_voxels=True), ml.voxels(), ml.dgraph(), ml.lethal(), ml.summary(), ml.reset()
    dl = depth_layer.DepthLayer(lp, depth_layer.shipped_config(max_markings=64), f32(5, 3), f32(3, 3))
    dl.update(T2)
    dl.voxels(), dl.clusters(), dl.dgraph(), dl.lethal(), dl.lethal_points(), dl.summary(), dl.reset()
    ps = stack.PerceptionStack(lp, ml, dl, host_layers=(None, np.arange(6, dtype=np.float64)), max_changes=8)
    ps.set_host_layer(0, np.ones(6))
    ps.set_host_layer(0, None)
    ps.update(T1, T2)
    ps.update()
    ps.n_changes(), ps.changes(), ps.min_dgraph(), ps.lethal_mask(), ps.lethal_nodes(), ps.summary(), ps.reset()
    pm = localization.ParticleMeasure(lp, localization.shipped_config(max_particles=64))
    pm.set_map(f32(4, 3), f32(3, 3), f32(3, 3, 2.0))
    pm.measure(f32(3, 3), f32(4, 4), f32(2, 7))
    pm.terms(2)
    pm.configure_observation(localization.shipped_observation_config(max_flat_points=8, max_less_sharp_points=8))
    pm.prepare(f32(3, 3), f32(4, 4), T34)
    pm.prepare_from_sweep(0, np.vstack([T34, [0, 0, 0, 1]]))
    pm.observation()
    pm.measure_prepared(f32(2, 7))

    # -- the cloud-taking methods once more, on empty inputs ---------------------------------------------------------------
    rec.calls.append(["-- empty inputs --"])
    none = np.zeros((0, 3), np.float32)
    feed(none, np.zeros((0, 4), np.float32), np.zeros((0, 6)))
    lp.depth_mark_create(0.05, 0.1, f32(4, 3), none)
    marking.MarkingLayer(lp, marking.shipped_config(), f32(5, 3), none)
    marking.MarkingLayer(lp, marking.shipped_config(), none, none)
    depth_layer.DepthLayer(lp, depth_layer.shipped_config(), f32(5, 3), none)
    pm.set_map(f32(4, 3), none, none)
    pm.measure(none, f32(4, 4), f32(2, 7))
    pm.measure(f32(3, 3), np.zeros((0, 4), np.float32), np.zeros((0, 7), np.float32))
    pm.prepare(none, f32(4, 4), T34)
    pm.prepare(f32(3, 3), none, T34)
    pm.measure_prepared(np.zeros((0, 7), np.float32))
    pm.configure_observation(None)
    return rec.calls


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--package-root", default=ROOT, help="the directory whose dddmr_navigation_amd is recorded")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root))
    calls = record()
    with open(a.out, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(c) for c in calls) + "\n]\n")
    print(f"{len(calls)} calls -> {a.out}")


if __name__ == "__main__":
    main()
