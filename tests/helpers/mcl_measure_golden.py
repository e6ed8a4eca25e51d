"""The particle-measure pin's cases by golden file, and the format of tests/golden/REF_MCL_*.npz (written by
tests/golden/make_ref_mcl_golden.py from the compiled reference's O2 build, read by the pin's CPU and GPU tests).

A file holds `names` and, per case i, under the prefix `c{i}_`: likelihood, quality (float32), trace ([N,8] float64, the
columns of oracle/ref_mcl_py.TRACE), branch (int32), quality_minmax (float32 [2]), cfg (float64 [4]: match_dist_min,
match_dist_flat, radius_of_ground_search, threshold_for_trusted_ground), draws, sha_<input> (the SHA-256 of each input
array's bytes, shape and type), and for the targeted cases the inputs themselves as in_<input>.  Every file also holds
gap_roll_ulp and gap_like_ulp: the largest difference between the reference's own O0 and O2 builds over all the pin's
particles, in double steps of roll and float steps of likelihood, measured when the files were written.
"""
from __future__ import annotations

import hashlib
import os

import numpy as np

import mcl_measure_ref as R
import mcl_measure_cases as Cs
import mcl_measure_pin_cases as Pc

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden")
INPUTS = ("map", "ground", "normals", "flat", "ls", "states")
OUTPUTS = ("likelihood", "quality", "trace", "branch", "quality_minmax")
NAMED = tuple(n for n in Cs.NAMES if n != "map-empty")          # (an empty map: the reference has no defined answer)


def _named(name):
    parts, ref, draws = Cs.case(name)
    return Cs.CFG, parts, ref, draws


def _known(name):
    for n, cfg, parts, _ in Cs.known_answers():
        if n == name:
            return cfg, parts, Cs.answer(parts, cfg), 1
    raise KeyError(name)


KNOWN = tuple(n for n, _, _, _ in Cs.known_answers())
# file name (without .npz) -> (case names, loader(name) -> (cfg, parts, restatement's answer, draws), inputs inline?)
FILES = {f"REF_MCL_{n}": ((n,), _named, False) for n in NAMED}
FILES["REF_MCL_known_answers"] = (KNOWN, _known, False)
FILES["REF_MCL_targeted"] = (tuple(Pc.TARGETED), Pc.case, True)
FILES["REF_MCL_rooms"] = (tuple(Pc.ROOMS), Pc.case, False)
CASES = tuple((f, n) for f, (names, _, _) in FILES.items() for n in names)


def load_case(file, name):
    """-> (cfg, parts, restatement's answer, draws), computed once per process"""
    return FILES[file][1](name)


def cfg_array(cfg):
    return np.array([cfg.match_dist_min, cfg.match_dist_flat, cfg.radius_of_ground_search, cfg.threshold_for_trusted_ground], np.float64)


def cfg_of(a):
    return R.Config(float(a[0]), float(a[1]), float(a[2]), int(a[3]))


def sha(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(repr((a.shape, a.dtype.str)).encode() + a.tobytes()).hexdigest()


def write(file, results, gap_roll_ulp, gap_like_ulp):
    """results: per case of the file, in order, the dict of oracle/ref_mcl_py.measure"""
    names, loader, inline = FILES[file]
    out = dict(names=np.array(names), gap_roll_ulp=np.int64(gap_roll_ulp), gap_like_ulp=np.int64(gap_like_ulp))
    for i, (name, res) in enumerate(zip(names, results)):
        cfg, parts, _, draws = loader(name)
        p = f"c{i}_"
        out[p + "likelihood"], out[p + "quality"] = res["likelihood"], res["quality"]
        out[p + "trace"], out[p + "branch"] = res["trace"], res["branch"]
        out[p + "quality_minmax"] = np.array([res["quality_min"], res["quality_max"]], np.float32)
        out[p + "cfg"], out[p + "draws"] = cfg_array(cfg), np.int64(draws)
        for k in INPUTS:
            out[p + "sha_" + k] = np.array(sha(parts[k]))
            if inline:
                out[p + "in_" + k] = parts[k]
    np.savez_compressed(os.path.join(GOLDEN, file + ".npz"), **out)


_open: dict = {}


def read(file, name):
    """-> dict of the stored arrays of one case, plus gap_roll_ulp / gap_like_ulp; AssertionError when the file is
    missing or does not list the case (the goldens are committed: regenerate with make_ref_mcl_golden.py)"""
    path = os.path.join(GOLDEN, file + ".npz")
    assert os.path.exists(path), f"{path} is missing: run tests/golden/make_ref_mcl_golden.py where the reference is built"
    if file not in _open:
        with np.load(path) as z:
            _open[file] = {k: z[k] for k in z.files}
    z = _open[file]
    names = [str(n) for n in z["names"]]
    assert name in names, f"{path} has no case {name}: regenerate it with tests/golden/make_ref_mcl_golden.py"
    p = f"c{names.index(name)}_"
    out = {k[len(p):]: v for k, v in z.items() if k.startswith(p)}
    out["gap_roll_ulp"], out["gap_like_ulp"] = int(z["gap_roll_ulp"]), int(z["gap_like_ulp"])
    return out


def check_inputs(file, name, parts, stored):
    """the inputs rebuilt here are the ones the golden was computed from, or the test fails and asks for regeneration"""
    for k in INPUTS:
        assert sha(parts[k]) == str(stored["sha_" + k]), \
            f"{file}: case {name}: input `{k}` rebuilt from the case generators differs from the one the golden was computed " \
            f"from; regenerate the goldens with tests/golden/make_ref_mcl_golden.py where the reference is built"
        if "in_" + k in stored:
            assert stored["in_" + k].tobytes() == np.ascontiguousarray(parts[k]).tobytes(), f"{file}: case {name}: stored input `{k}`"


def ulps32(a, b):
    """distance in float32 steps; two NaNs are 0 apart, a NaN and a number 2^40"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia), np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    d = np.abs(ia - ib)
    na, nb = np.isnan(a), np.isnan(b)
    return np.where(na | nb, np.where(na & nb, 0, 1 << 40), d)


def ulps64(a, b):
    """distance in float64 steps, computed in Python integers; NaNs as in ulps32"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    out = np.zeros(a.shape, np.int64).ravel()
    for i, (x, y) in enumerate(zip(a.ravel(), b.ravel())):
        if np.isnan(x) or np.isnan(y):
            out[i] = 0 if (np.isnan(x) and np.isnan(y)) else 1 << 40
            continue
        ix, iy = int(np.float64(x).view(np.int64)), int(np.float64(y).view(np.int64))
        ix, iy = (-(ix & 0x7FFFFFFFFFFFFFFF) if ix < 0 else ix), (-(iy & 0x7FFFFFFFFFFFFFFF) if iy < 0 else iy)
        out[i] = min(abs(ix - iy), 1 << 40)
    return out.reshape(a.shape)
