#!/usr/bin/env python3
"""Checks the variant-(ii) patches against a checkout of the reference (not part of the test suite, which runs from
this repository alone):

* all four patches apply to the checkout without fuzz, and the committed files are what make_patches.py generates
  from it;
* g++ -fsyntax-only against the stand-in headers of tests/stubs/ passes for the three adapter sources and for the four
  reference files as the patches leave them, and the check can fail (a call the patched planner does not have is
  caught).

usage: python tools/check_adapter_patches.py REFERENCE_CHECKOUT        (needs patch(1) and g++)"""
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AD = os.path.join(ROOT, "adapters", "ros2")


def patched_tree(ref, tmp):
    """A copy of the reference packages the patches touch, with every patch applied -> [(patch, CompletedProcess)]."""
    for pkg, subs in (("dddmr_local_planner", ("local_planner", "recovery_behaviors")), ("dddmr_perception_3d", ("include", "plugins", "src"))):
        for sub in subs:
            shutil.copytree(os.path.join(ref, "src", pkg, sub), os.path.join(tmp, "src", pkg, sub))
    out = []
    for p in sorted(os.listdir(os.path.join(AD, "patches"))):
        if p.endswith(".patch"):
            out.append((p, subprocess.run(["patch", "-p1", "-i", os.path.join(AD, "patches", p)], cwd=tmp, capture_output=True, text=True)))
    return out


def check_apply(ref):
    with tempfile.TemporaryDirectory() as tmp:
        res = patched_tree(ref, tmp)
        assert len(res) == 4
        for p, r in res:
            assert r.returncode == 0, (p, r.stdout, r.stderr)
            assert "FAILED" not in r.stdout and "fuzz" not in r.stdout, r.stdout
    with tempfile.TemporaryDirectory() as tmp:
        shutil.copytree(os.path.join(AD, "patches"), os.path.join(tmp, "patches"))
        r = subprocess.run([sys.executable, os.path.join(tmp, "patches", "make_patches.py"), ref], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        for p in os.listdir(os.path.join(AD, "patches")):
            if p.endswith(".patch"):
                assert open(os.path.join(tmp, "patches", p)).read() == open(os.path.join(AD, "patches", p)).read(), p + " is stale"


def check_syntax(ref):
    stubs = os.path.join(ROOT, "tests", "stubs")
    with tempfile.TemporaryDirectory() as tmp:
        shutil.copytree(os.path.join(ref, "src", "dddmr_sys_core", "include"), os.path.join(tmp, "src", "dddmr_sys_core", "include"))
        for sub in ("trajectory_generators", "mpc_critics", "base_trajectory"):
            shutil.copytree(os.path.join(ref, "src", "dddmr_local_planner", sub, "include"), os.path.join(tmp, "src", "dddmr_local_planner", sub, "include"))
        for p, r in patched_tree(ref, tmp):
            assert r.returncode == 0, (p, r.stdout, r.stderr)
        src = os.path.join(tmp, "src")
        inc = ["-I", stubs, "-I", os.path.join(ROOT, "include"), "-I", os.path.join(AD, "dddmr_rollout_adapter", "include")]
        for d in ("dddmr_local_planner/trajectory_generators", "dddmr_local_planner/mpc_critics", "dddmr_local_planner/base_trajectory",
                  "dddmr_sys_core", "dddmr_perception_3d", "dddmr_local_planner/local_planner", "dddmr_local_planner/recovery_behaviors"):
            inc += ["-I", os.path.join(src, d, "include")]
        files = [os.path.join(AD, "dddmr_rollout_adapter", "src", f) for f in sorted(os.listdir(os.path.join(AD, "dddmr_rollout_adapter", "src")))]
        files += [os.path.join(src, f) for f in ("dddmr_local_planner/local_planner/src/local_planner.cpp",
                                                  "dddmr_local_planner/recovery_behaviors/behaviors/rotate_inplace_behavior.cpp",
                                                  "dddmr_perception_3d/plugins/multilayer_spinning_lidar.cpp",
                                                  "dddmr_perception_3d/plugins/path_blocked_strategy.cpp")]
        assert len(files) == 7
        procs = [(f, subprocess.Popen(["g++", "-std=c++17", "-fsyntax-only", "-w"] + inc + [f], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
                 for f in files]
        for f, pr in procs:
            _, err = pr.communicate()
            assert pr.returncode == 0, (f, err[-3000:])
        bad = os.path.join(tmp, "bad.cpp")
        open(bad, "w").write(open(files[3]).read().replace("dddmr_rollout_adapter::rolloutTick(", "dddmr_rollout_adapter::rolloutTock(", 1))
        r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-w"] + inc + [bad], capture_output=True, text=True)
        assert r.returncode != 0 and "rolloutTock" in r.stderr


if __name__ == "__main__":
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "src", "dddmr_local_planner")):
        sys.exit(__doc__)
    check_apply(sys.argv[1])
    check_syntax(sys.argv[1])
    print("adapter patches: apply cleanly, up to date, syntax OK")
