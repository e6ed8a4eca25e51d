"""The ROS 2 adapter sources (adapters/ros2/) cannot be compiled here (no ROS 2 / PCL / pluginlib in the
image), so this checks what can be checked: every C-ABI symbol, enum and struct field they use exists in
include/dddmr_rollout.h, the plugin manifest names the classes the sources export, and the variant-(ii) patches are
well-formed unified diffs whose added lines make the adapter calls."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from conftest import ROOT

AD = os.path.join(ROOT, "adapters", "ros2")


def _sources():
    out = {}
    for d, _, files in os.walk(AD):
        for f in files:
            if f.endswith((".h", ".cpp", ".patch")):
                out[os.path.join(d, f)] = open(os.path.join(d, f)).read()
    return out


def test_adapter_sources_only_use_declared_abi():
    header = open(os.path.join(ROOT, "include", "dddmr_rollout.h")).read()
    declared = set(re.findall(r"\b(dddmr_rollout_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    types = set(re.findall(r"\b(dddmr_[a-z_]+)\b", header))
    macros = set(re.findall(r"\b(DDDMR_[A-Z_0-9]+)\b", header))
    srcs = _sources()
    assert len(srcs) >= 8
    for path, text in srcs.items():
        added = "\n".join(l[1:] for l in text.split("\n") if l.startswith("+")) if path.endswith(".patch") else text
        for call in set(re.findall(r"\b(dddmr_rollout_[a-z_]+)\s*\(", added)):
            assert call in declared, (path, call)
        for name in set(re.findall(r"\b(dddmr_[a-z_]+)\b", added)):
            if name.startswith("dddmr_rollout_adapter") or name in ("dddmr_sys_core", "dddmr_navigation", "dddmr_local_planner",
                                                                     "dddmr_navigation_amd", "dddmr_p", "dddmr_rollout"):
                continue
            assert name in types or name in declared, (path, name)
        for m in set(re.findall(r"\b(DDDMR_[A-Z_0-9]+)\b", added)):
            if m.startswith("DDDMR_ROLLOUT_ADAPTER") or m in ("DDDMR_ROLLOUT_ROOT", "DDDMR_ROLLOUT_LIB"):
                continue
            assert m in macros, (path, m)
    # struct fields the adapters fill exist in the header
    bridge = srcs[os.path.join(AD, "dddmr_rollout_adapter", "src", "gpu_rollout_theory.cpp")]
    for field in set(re.findall(r"config_\.([a-z_]+)", bridge)):
        assert re.search(r"\b%s\b" % field, header), field


def test_plugin_manifest_matches_exported_classes():
    xml = open(os.path.join(AD, "dddmr_rollout_adapter", "plugins.xml")).read()
    srcs = _sources()
    exported = set()
    for path, text in srcs.items():
        if not path.endswith(".patch"):       # (patches quote the reference's own export lines as context)
            exported |= set(re.findall(r"PLUGINLIB_EXPORT_CLASS\((\S+?),", text))
    assert exported == set(re.findall(r'class type="([^"]+)"', xml)) and len(exported) == 2
    assert "trajectory_generators::TrajectoryGeneratorTheory" in xml and "mpc_critics::ScoringModel" in xml


def _patch_files(text):
    """{path: [(old_start, old_len, new_start, new_len, [hunk lines])]} of a unified diff, headers checked."""
    files, path, hunk = {}, None, None
    lines = text.split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    i = 0
    while i < len(lines):
        l = lines[i]
        if l.startswith("--- a/"):
            assert lines[i + 1] == "+++ b/" + l[len("--- a/"):], (l, lines[i + 1])
            path = l[len("--- a/"):]
            assert path not in files, path
            files[path] = []
            hunk = None
            i += 2
            continue
        m = re.match(r"@@ -(\d+),(\d+) \+(\d+),(\d+) @@", l)
        if m:
            assert path is not None, l
            hunk = tuple(int(g) for g in m.groups()) + ([],)
            files[path].append(hunk)
        else:
            assert hunk is not None and l[:1] in (" ", "+", "-"), l
            hunk[4].append(l)
        i += 1
    return files


def test_variant_ii_patches_are_well_formed():
    """Planner (local_planner.cpp:535-587), second caller (rotate_inplace_behavior.cpp:224-259) and the perception side
    (multilayer_spinning_lidar.cpp, path_blocked_strategy.cpp): every hunk header counts its own lines, the hunks of a
    file are in order without overlap and their new-side offsets follow from the lines added before them, and the added
    lines make the adapter calls (make_patches.py regenerates the patches from a reference checkout)."""
    added = {}
    names = sorted(p for p in os.listdir(os.path.join(AD, "patches")) if p.endswith(".patch"))
    assert len(names) == 4
    for p in names:
        files = _patch_files(open(os.path.join(AD, "patches", p)).read())
        assert files, p
        for path, hunks in files.items():
            assert path.startswith("src/") and hunks, (p, path)
            shift, end = 0, 0
            for o0, on, n0, nn, body in hunks:
                assert sum(l[0] in " -" for l in body) == on and sum(l[0] in " +" for l in body) == nn, (p, path, o0)
                assert o0 > end and n0 == o0 + shift, (p, path, o0)
                assert any(l[0] != " " for l in body), (p, path, o0)
                shift += nn - on
                end = o0 + on - 1
            added[path] = "\n".join(l[1:] for _, _, _, _, body in hunks for l in body if l[0] == "+")
    lidar = added["src/dddmr_perception_3d/plugins/multilayer_spinning_lidar.cpp"]
    for call in ("feedScan(", "gpu_marking_.clearThenMark(", "gpu_marking_.create(", "gpu_marking_.dGraphValue(", "gpu_marking_.lethalPointCloud("):
        assert call in lidar, call
    assert "dddmr_rollout_adapter::pathBlocked(" in added["src/dddmr_perception_3d/plugins/path_blocked_strategy.cpp"]
    planner = added["src/dddmr_local_planner/local_planner/src/local_planner.cpp"]
    assert "dddmr_sys_core::PERCEPTION_MALFUNCTION" in planner.split("rolloutTick(")[1]
    assert "rolloutTick(" in added["src/dddmr_local_planner/recovery_behaviors/behaviors/rotate_inplace_behavior.cpp"]


def test_bridges_compile_and_behave_without_ros():
    """planner_bridge.h / perception_bridge.h / shared_context.h are templates over the ROS / PCL types: compiled here
    with stand-in types against a fake C-ABI (tests/cpp/adapter_bridge_test.cpp) and run -- a rejected observation never
    lets the tick run, a failed tick is an engine error (not "all trajectories fail"), a device feed is not overwritten."""
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "adapter_bridge_test")
        r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                            "-I", os.path.join(AD, "dddmr_rollout_adapter", "include"),
                            os.path.join(ROOT, "tests", "cpp", "adapter_bridge_test.cpp"), "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and "adapter bridges OK" in r.stdout, (r.stdout, r.stderr)
