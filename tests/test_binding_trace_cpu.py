"""What the Python binding hands to the C library is pinned to a recording: tools/binding_trace.py replays its script of
every public method on a stand-in library, and the calls must equal tests/golden/binding_trace.json, recorded from the
package as it was before the binding moved to _capi.SIGNATURES and _marshal (the tool's docstring says how).  Needs no
library and no GPU."""
import importlib.util
import json
import os

from conftest import ROOT

# The only differences from the recording: an EMPTY cloud argument goes to the library as (null pointer, 0, stride 12)
# whatever the method; the recording has a pointer to no element there, and a stride of 16 (set_cloud) or 0 (mcl_prepare).
# function -> (positions of its cloud pointers in the call, the line of C that makes pointer and stride irrelevant at a
# count of 0).  cloud_arg_ok is point_grid_plan.hip.h: `return !n || (xyz && stride_bytes >= 12 && stride_bytes % 4 == 0);`
# and no entry point reads a record or uses the stride outside a loop over the count.
EMPTY_CLOUD = {
    "set_cloud": ((2,), "rollout_engine.hip: if (!cloud_arg_ok(xyzi, n_points, stride_bytes)) return fail(...)"),
    "set_scan": ((2,), "sensor_sources.hip.h set_scan_impl: if (!cloud_arg_ok(xyz, n_points, stride_bytes)) return fail(...)"),
    "set_scan_source": ((3,), "sensor_sources.hip.h set_scan_impl: the same line"),
    "set_depth_frame": ((3,), "sensor_sources.hip.h: if (!cloud_arg_ok(xyz, n_points, stride_bytes)) return fail(...)"),
    "set_lidar_sweep": ((3,), "sensor_sources.hip.h: if (!cloud_arg_ok(xyz, n_points, stride_bytes)) return fail(...)"),
    "depth_frustum_test": ((2,), "sensor_sources.hip.h: if (n == 0) return DDDMR_OK;  (before xyz is read)"),
    "marking_create": ((3, 6), "marking_host.hip.h: if (!cloud_arg_ok(ground_xyz, ...) || !cloud_arg_ok(map_xyz, ...)) return fail(...)"),
    "mcl_prepare": ((2, 5), "mcl_observation.hip.h: if (!T_b2s || !cloud_arg_ok(flat_xyz, ...) || !cloud_arg_ok(less_sharp_xyz, ...))"),
}
MARK = ["-- empty inputs --"]


def _tool():
    spec = importlib.util.spec_from_file_location("binding_trace", os.path.join(ROOT, "tools", "binding_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _as_decided(call):
    """A recorded call with its empty cloud arguments in the form decided for them."""
    call = list(call)
    for p in EMPTY_CLOUD.get(call[0], ((), ""))[0]:
        if call[p + 1] == 0:
            assert call[p] in ("", "null"), call
            call[p: p + 3] = ["null", 0, 12]
    return call


def test_every_call_matches_the_recording():
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "binding_trace.json")))
    got = json.loads(json.dumps(_tool().record()))
    assert [c[0] for c in got] == [c[0] for c in want]
    cut = want.index(MARK)
    assert got.index(MARK) == cut and cut > 100
    for i, (g, w) in enumerate(zip(got, want)):
        if i < cut:
            assert g == w, f"call {i} ({w[0]}) differs from the recording"
        else:
            assert g == _as_decided(w), f"call {i} ({w[0]}, empty input) differs from the recording"
    differing = sorted({w[0] for g, w in zip(got, want) if g != w})
    assert differing == sorted(EMPTY_CLOUD), differing


def test_the_recording_covers_the_public_methods():
    """every public method of the five classes is in the script (so a new one has to be added to it)"""
    import inspect
    from dddmr_navigation_amd import depth_layer, localization, marking, stack
    from dddmr_navigation_amd.local_planner import LocalPlanner
    script = inspect.getsource(_tool().record)
    for cls in (LocalPlanner, marking.MarkingLayer, depth_layer.DepthLayer, stack.PerceptionStack, localization.ParticleMeasure):
        for name, _ in inspect.getmembers(cls, inspect.isfunction):
            if name.startswith("depth_layer_"):
                continue                                   # (LocalPlanner's half of DepthLayer: reached through its methods)
            if not name.startswith("_") and name not in ("close", "set_prune_plan"):
                assert f".{name}(" in script, f"{cls.__name__}.{name} is not in tools/binding_trace.py's script"
