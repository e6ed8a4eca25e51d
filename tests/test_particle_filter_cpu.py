"""The particle filter's host side, without a GPU:
1. the NumPy restatement (tests/helpers/particle_filter_ref.py) against the answers of mcl_3dl's OWN pf.h / state_6dof.h /
   motion model, recorded stage by stage by tools/record_pf_golden.* into tests/golden/REF_MCL_PF_N*.npz: bit for bit;
2. the plan header (csrc/mcl_filter_plan.hip.h: setOdoms, NormalLikelihood's constants, Quat(front, up), getMean) built
   with a plain host compiler against the restatement, once plain and once as a stand-alone program under
   AddressSanitizer + UndefinedBehaviorSanitizer;
3. the bridge's draw helpers (particle_filter_bridge.h) against the draws the reference's engine made;
4. the binding's signature table and struct layouts."""
import ctypes as C
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from dddmr_navigation_amd import _capi as K
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import particle_filter_ref as R  # noqa: E402
import particle_filter_cases as Cs  # noqa: E402
import capi_header  # noqa: E402

F = np.float32
CSRC = os.path.join(ROOT, "dddmr_navigation_amd", "csrc")
CXX = shutil.which("g++") or shutil.which("c++")
needs_cxx = pytest.mark.skipif(CXX is None, reason="needs a C++ compiler")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b, what):
    a, b = np.asarray(a, F), np.asarray(b, F)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.argwhere(bits(a) != bits(b))
    assert len(bad) == 0, (what, f"{len(bad)} of {a.size} differ", tuple(bad[0]), a[tuple(bad[0])], b[tuple(bad[0])])


# ---- 1. the restatement against the reference's recorded answers -------------------------------------------------------
@pytest.mark.parametrize("n", Cs.GOLDEN_SIZES)
def test_restatement_matches_the_reference_at_every_stage(n):
    g = Cs.golden(n)
    assert len(g["in_states"]) == n and (n <= 16 or int(g["resample_ties"][0]) == 0)
    dt, lin_tc, ang_tc = g["predict_params"]
    o = R.set_odoms(g["odom_prev"], g["odom_cur"], dt, lin_tc, ang_tc)
    s = R.predict(g["in_states"], g["in_noise4"], o)
    same(s, g["predict_states"], "predict")
    same(g["in_noise4"], g["predict_noise4"], "predict leaves the noise")
    p, total, restored = R.weigh(g["in_probability"], g["likelihood"])
    assert restored == 0 and total > 0
    same(p, g["measure_probability"], "pf::measure")
    b = R.bias(s, g["state_prev"], *g["bias_params"])
    same(b, g["measure_bias"], "bias")
    broke = False
    for stage in ("measure", "scaled"):
        e = R.estimate(g[stage + "_states"], g[stage + "_probability"], g[stage + "_bias"])
        same(e["mean_biased"], g[stage + "_mean_biased"], stage + ": expectationBiased")
        same(e["mean"], g[stage + "_mean"], stage + ": expectation(1.0)")
        same(e["max_state"], g[stage + "_max_state"], stage + ": max")
        same(e["cov"], g[stage + "_cov"], stage + ": covariance")
        broke |= e["p_num"] < n
    assert broke or n <= 2                                # the scaled set stops expectation(1.0) inside the array
    rows = np.stack([R.noise_row(d) for d in g["resample_draws"]])
    r = R.resample(g["measure_states"], g["measure_noise4"], g["measure_probability"], g["resample_u"][0], rows)
    same(r["states"], g["resample_states"], "resample: states")
    same(r["noise4"], g["resample_noise4"], "resample: noise")
    same(r["probability"], g["resample_probability"], "resample: probabilities")
    assert r["n_ties"] == int(g["resample_ties"][0]) and r["n_duplicates"] > 0
    s2, z2 = R.add_noise(g["resample_states"], np.stack([R.noise_row(d) for d in g["add_noise_draws"]]))
    same(s2, g["add_noise_states"], "pf::noise: states")
    same(z2, g["add_noise_noise4"], "pf::noise: noise")
    same(g["resample_probability"], g["add_noise_probability"], "pf::noise leaves the probabilities")


def test_goldens_are_small():
    for n in Cs.GOLDEN_SIZES:
        assert os.path.getsize(os.path.join(Cs.GOLDEN, f"REF_MCL_PF_N{n}.npz")) < (1 << 20)


def test_resample_restatement_properties():
    """the end() branch keeps the last valid pick; a refused row count leaves no states; the lowest index wins a tie"""
    n = 100
    s, z = Cs.particles(n)
    p = Cs.probability(n, "normalised")
    r = R.resample(s, z, p, Cs.U_MAX, Cs.noise_rows(n))
    assert r["n_at_end"] >= 1 and (r["pick"][n - r["n_at_end"]:] == r["pick"][n - r["n_at_end"] - 1]).all()
    assert R.resample(s, z, p, 0.0, Cs.noise_rows(n)[: r["n_duplicates"] - 1])["states"] is None or r["n_duplicates"] == 0
    p = np.array([0.5, 0, 0, 0.5, 0, 0], F)
    r = R.resample(s[:6], z[:6], p, 0.5, Cs.noise_rows(6))
    assert r["n_ties"] == 4 and set(r["pick"]) == {0, 3}


# ---- 2. the plan header ------------------------------------------------------------------------------------------------
def hexes(v):
    return " ".join(f"{int(b):08x}" for b in bits(np.asarray(v, F).ravel()))


def plan_lines():
    """(input line, expected floats) pairs"""
    out = []
    rng = np.random.default_rng(5)
    odoms = [(Cs.ODOM_PREV, Cs.ODOM_CUR, Cs.DT), (Cs.ODOM_PREV, Cs.ODOM_PREV, 0.05)]          # (no motion: getAxisAng's first branch)
    back = Cs.ODOM_PREV.copy()
    back[3:7] = R.qmul(R.quat_from_rpy(np.array([0, 0, 3.5], F)), Cs.ODOM_PREV[3:7])           # (an angle beyond pi)
    odoms.append((Cs.ODOM_PREV, back, 0.2))
    for n in Cs.GOLDEN_SIZES[:2]:
        g = Cs.golden(n)
        odoms.append((g["odom_prev"], g["odom_cur"], g["predict_params"][0]))
    for a, b, dt in odoms:
        o = R.set_odoms(a, b, dt, Cs.LIN_TC, Cs.ANG_TC)
        want = np.concatenate([o["rt"], o["rq"], [o["rt_norm"], o["rel_ang"], o["decay_lin"], o["decay_ang"]]])
        out.append(("odoms " + hexes(np.concatenate([a, b, [dt, Cs.LIN_TC, Cs.ANG_TC]])), want))
    for sigma in (Cs.VAR_DIST, Cs.VAR_ANG, 0.013, 250.0):
        out.append(("nl " + hexes([sigma]), np.array(R.normal_likelihood(sigma), F)))
    for _ in range(8):
        f, u = rng.standard_normal(3).astype(F), rng.standard_normal(3).astype(F)
        out.append(("axes " + hexes(np.concatenate([f, u])), R.quat_from_axes(f, u)))
    for f, u in (([1, 0, 0], [0, 0, 1]), ([-1, 0, 0], [0, 0, 1]), ([0, 1, 0], [0, 0, -1]), ([0, 0, 0], [0, 0, 1])):   # (the last: NaN axes -> max(0.0, NaN))
        out.append(("axes " + hexes(np.array(f + u, F)), R.quat_from_axes(np.array(f, F), np.array(u, F))))
    for n in (2, 60):
        g = Cs.golden(n)
        sums = R.ordered_sums(R.mean_terms(g["measure_states"], (g["measure_probability"] * g["measure_bias"]).astype(F)))
        out.append(("mean " + hexes(sums), R.mean_from_sums(sums)))
    a_l, q_l = R.normal_likelihood(Cs.VAR_DIST)
    a_a, q_a = R.normal_likelihood(Cs.VAR_ANG)
    want = np.concatenate([Cs.STATE_PREV[:3], R.qinv(Cs.STATE_PREV[3:7]), [a_l, q_l, a_a, q_a]])
    out.append(("bias " + hexes(np.concatenate([Cs.STATE_PREV, [Cs.VAR_DIST, Cs.VAR_ANG]])), want))
    return out


def build_plan_test(tmp, *flags):
    exe = os.path.join(tmp, "mcl_filter_plan_test" + ("_san" if flags else ""))
    r = subprocess.run([CXX, "-x", "c++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC,
                        os.path.join(ROOT, "tests", "cpp", "mcl_filter_plan_test.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def check_plan(exe):
    lines = plan_lines()
    r = subprocess.run([exe], input="\n".join(l for l, _ in lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr)
    got = r.stdout.strip().split("\n")
    assert len(got) == len(lines)
    for (line, want), g in zip(lines, got):
        g = np.array([int(t, 16) for t in g.split()], np.uint32)
        w = bits(want)
        nan = np.isnan(np.asarray(want, F))
        assert len(g) == len(w) and (g[~nan] == w[~nan]).all() and np.isnan(g[nan].view(F)).all(), (line, g, w)


@needs_cxx
def test_plan_header_matches_the_restatement():
    with tempfile.TemporaryDirectory() as tmp:
        check_plan(build_plan_test(tmp))


@needs_cxx
def test_plan_header_under_the_sanitizers():
    with tempfile.TemporaryDirectory() as tmp:
        check_plan(build_plan_test(tmp, "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


# ---- 3. the bridge's draws ---------------------------------------------------------------------------------------------
@needs_cxx
def test_bridge_draws_are_the_references_draws():
    inc = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "adapters", "ros2", "dddmr_rollout_adapter", "include")]
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "particle_filter_bridge_test")
        r = subprocess.run([CXX, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *inc,
                            os.path.join(ROOT, "tests", "cpp", "particle_filter_bridge_test.cpp"), "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        for n in (2, 17, 60):
            g = Cs.golden(n)
            rows = np.stack([R.noise_row(d) for d in g["resample_draws"]])
            ref = R.resample(g["measure_states"], g["measure_noise4"], g["measure_probability"], g["resample_u"][0], rows)
            # (the recorder seeds the filter's engine with 20240521 + n and draws nothing before resample)
            r = subprocess.run([exe, str(20240521 + n), str(n), str(ref["n_duplicates"])], capture_output=True, text=True)
            assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
            out = r.stdout.split()
            assert int(out[0], 16) == int(bits(g["resample_u"])[0]), "the canonical draw"
            got = np.array([int(t, 16) for t in out[1:1 + 10 * n]], np.uint32).reshape(n, 10)
            assert (got == bits(rows)).all(), "the noise rows"
            assert int(out[1 + 10 * n]) == int(g["engine_after_resample"][0]), "the engine after 6 * n_duplicates normal draws"


# ---- 4. the binding ----------------------------------------------------------------------------------------------------
def test_signatures_and_struct_layouts():
    protos = capi_header.prototypes()
    names = ["create", "set_particles", "get_particles", "predict", "set_noise", "measure", "reset_integ", "resample", "add_noise"]
    for name in ("dddmr_rollout_mcl_filter_" + n for n in names):
        assert name in K.SIGNATURES and name in K.EXPORTED_SYMBOLS and name in protos, name
        restype, argtypes = K.SIGNATURES[name]
        ret, params = protos[name]
        assert capi_header.ctypes_kind(restype, True) == ret == "int" and len(argtypes) == len(params), name
        for t, kind in zip(argtypes, params):
            assert capi_header.ctypes_kind(t) == ("ptr" if kind in ("in", "out") else kind), (name, kind)
    assert (C.sizeof(K.MclFilterConfig), C.sizeof(K.MclFilterEstimate), C.sizeof(K.MclFilterResampleStats)) == (40, 368, 24)
    text = open(os.path.join(CSRC, "mcl_filter.hip.h")).read()
    assert "sizeof(dddmr_mcl_filter_config) == 40 && sizeof(dddmr_mcl_filter_estimate) == 368 && sizeof(dddmr_mcl_filter_resample_stats) == 24" in text
    header = open(capi_header.HEADER).read()
    for cls, name in ((K.MclFilterConfig, "dddmr_mcl_filter_config"), (K.MclFilterEstimate, "dddmr_mcl_filter_estimate"),
                      (K.MclFilterResampleStats, "dddmr_mcl_filter_resample_stats")):
        body = header[: header.index("} " + name + ";")]
        body = body[body.rindex("typedef struct {"):]
        at = 0
        for field, _ in cls._fields_:                      # the fields appear in the header in the mirror's order
            at = body.index(field, at) + 1
