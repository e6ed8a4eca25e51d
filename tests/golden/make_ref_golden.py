"""Generates tests/golden/REF_*.npz from the reference's own rollout code, compiled from a reference checkout
(`make -C oracle ref`, oracle/_ref/libref_O2.so; see oracle/ref/ref_driver.cpp), so that the pin travels without the
reference: the oracle must reproduce every REF_* bit (tests/test_reference_pin_cpu.py) and the HIP path must match
them within the parity bar (tests/test_reference_pin_gpu.py).

Each file holds its inputs (theory and tick-input bytes, cloud, plan) and the keys of make_golden.py.  The reference
has no margin output, so `min_margin` (the fragile-point rule of the GPU parity check) is the oracle's on the same
scene; the CPU pin shows the two agree on every verdict.  `poses` / `poses_index`: per-step poses of a few generated
trajectories.  Scenes with a bench-mode theory are run with the bench extensions off (the reference has none).

Run from the repo root:  python tests/golden/make_ref_golden.py
"""
import ctypes as C
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from dddmr_navigation_amd import _capi as K, configs, scenes  # noqa: E402
import oracle  # noqa: E402
from oracle import ref_py as R  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def ref_scenes():
    out = {}
    for goal, tag in (((3.0, 1.0), "L"), ((3.0, -1.0), "R")):
        for st, stag in ((5.0, "st5"), (2.0, "st2")):
            out[f"REF_F1_playground_{tag}_{stag}"] = scenes.playground_scene(goal, st)
    sc = scenes.bench_scene("C1")
    sc.theory.bench_fixed_steps = 0
    sc.theory.bench_no_zero_insert = 0
    out["REF_F6_C1"] = sc
    cloud = scenes.cloud_c1(seed=41, n_points=3000)
    plan = scenes.s_curve_plan()
    dd = configs.dd_simple_shipped(name="ref_dd", linear_x_sample=6.0, angular_z_sample=9.0, max_vel_x=1.0,
                                   acc_lim_x=2.0, max_vel_theta=0.8, acc_lim_theta=3.0)
    omni = configs.omni_simple_shipped(name="ref_omni", linear_x_sample=5.0, linear_y_sample=4.0, angular_z_sample=5.0)
    rot = configs.rotate_inplace_shipped("ref_rotate", shortest=True)
    out["REF_R1_dd"] = scenes.Scene("dd", dd, cloud, plan, scenes.tick_input(twist=(0.5, 0.0, 0.2)))
    out["REF_R2_omni"] = scenes.Scene("omni", omni, cloud, plan, scenes.tick_input(twist=(0.05, -0.03, 0.0)))
    out["REF_R3_rotate"] = scenes.Scene("rotate", rot, cloud, plan,
                                        scenes.tick_input(twist=(0.0, 0.0, 0.3), heading_deviation=-math.pi))
    q = scenes.quat_from_rpy(math.radians(3.0), math.radians(-6.0), 2.9)
    out["REF_R4_tilted"] = scenes.Scene("tilted", dd, cloud, plan, scenes.tick_input(pose=(0.2, -0.1, 0.05) + tuple(q)))
    off = np.array([2500.0, -1200.0, 3.0], np.float32)
    cloud_off = cloud.copy()
    cloud_off[:, :3] += off
    plan_off = plan.copy()
    plan_off[:, :3] += off.astype(np.float64)
    q = scenes.quat_from_rpy(0.0, 0.0, -3.1)
    out["REF_R5_offset"] = scenes.Scene("offset", dd, cloud_off, plan_off,
                                        scenes.tick_input(pose=tuple(off.astype(np.float64)) + tuple(q), allowed_max=0.45))
    # F9's situation on a small cloud: the robot pitched 10 degrees, cuboids tilted out of the grid's axes
    q = scenes.quat_from_rpy(0.0, math.radians(10.0), 0.4)
    out["REF_R6_pitched"] = scenes.Scene("pitched", dd, cloud, plan, scenes.tick_input(pose=(0.0, 0.0, 0.0) + tuple(q)))
    out["REF_R7_omni_step_boundary"] = omni_step_boundary_scene(cloud, plan)
    return out


def omni_step_boundary_scene(cloud, plan):
    """Omni scene whose sim_granularity puts one sample's step count exactly between the float hypot the reference
    computes (omni_simple...cpp:387, ASSUMPTIONS.md row 18) and a double hypot: the steps differ by one if a port
    uses the double hypot, or rounds the float one differently."""
    st = 2.0
    omni = configs.omni_simple_shipped(name="ref_omni_boundary", linear_x_sample=5.0, linear_y_sample=4.0,
                                       angular_z_sample=3.0, sim_time=st, angular_sim_granularity=10.0)
    ti = scenes.tick_input(twist=(0.05, -0.03, 0.0))
    best = None
    for s in oracle.samples(omni, ti):
        vf = float(np.hypot(s[0], s[1]))                   # float hypot (glibc hypotf), widened
        vd = math.hypot(float(s[0]), float(s[1]))
        if vf != vd and vd > 0.05 and (best is None or abs(vf - vd) / vd > best[0]):
            best = (abs(vf - vd) / vd, vf, vd)
    _, vf, vd = best
    k = 37
    omni.sim_granularity = st * (vf + vd) / 2.0 / k        # vf * st / g and vd * st / g straddle k
    assert math.ceil(vf * st / omni.sim_granularity) != math.ceil(vd * st / omni.sim_granularity)
    return scenes.Scene("omni_step_boundary", omni, cloud, plan, ti)


def dump(name, sc):
    r, costs, steps, smp = R.tick(sc.theory, sc.cloud, sc.plan, sc.tick, build="O2")
    o = oracle.tick(sc.theory, sc.cloud, sc.plan, sc.tick, n_threads=8, want_margin=True)
    gen = np.nonzero(steps > 0)[0]
    pick = gen[np.linspace(0, len(gen) - 1, min(4, len(gen))).astype(int)] if len(gen) else gen
    poses = [R.generate(sc.theory, sc.tick, smp[i], build="O2")[0] for i in pick]
    np.savez_compressed(
        os.path.join(HERE, name + ".npz"),
        theory=np.frombuffer(bytes(sc.theory), np.uint8), tick=np.frombuffer(bytes(sc.tick), np.uint8),
        cloud=np.ascontiguousarray(sc.cloud, np.float32), plan=np.ascontiguousarray(sc.plan, np.float64),
        costs=costs, steps=steps, samples=smp, min_margin=o.min_margin,
        summary=np.array([r.planner_state, r.best_index, r.n_samples, r.n_generated], dtype=np.int64),
        best=np.array([r.best_cost, r.vx, r.vy, r.wz], dtype=np.float64),
        poses=np.concatenate(poses) if poses else np.zeros((0, 7)), poses_index=pick.astype(np.int32),
        poses_count=np.array([len(p) for p in poses], np.int32))
    print(f"{name}: N={r.n_samples} generated={r.n_generated} best={r.best_index} cost={r.best_cost:.9f}")


def load(path):
    """-> (theory, tick, cloud, plan, npz) of a REF_* file."""
    g = np.load(path)
    th = K.TheoryConfig.from_buffer_copy(g["theory"].tobytes())
    ti = K.TickInput.from_buffer_copy(g["tick"].tobytes())
    return th, ti, g["cloud"], g["plan"], g


def main():
    for name, sc in ref_scenes().items():
        dump(name, sc)


if __name__ == "__main__":
    main()
