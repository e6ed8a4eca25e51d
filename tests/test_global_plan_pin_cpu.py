"""The planner pin: tests/helpers/global_plan_ref.py against the reference's own a_star_on_pre_graph.cpp and
static_graph.cpp, compiled unmodified against oracle/ref/shim/ (`make -C oracle ref`, oracle/ref/ref_gp_driver.cpp).

Live part (skipped where oracle/_ref/libref_gp_*.so is absent): the restatement, run with libm's own exp (math.exp, element
by element: NumPy's vector exp need not be glibc's) and libm's own acosf (the reference's theta),
against the O0 build on bits: path and status, every opened node's g, f, parent and closed flag, the closed count, the
final size of the set, and theta on more than 100 000 triples.  The reference's own O0-to-O2 gap is measured over all cases
and the restatement held to the O2 build within exactly that.  Every case sent to the reference also goes, in one file,
through oracle/_ref/ref_gp_asan, the same driver as a stand-alone program under AddressSanitizer and UBSan, which must
exit 0: no pinned case reaches the read of an emptied set's begin() (a_star_on_pre_graph.cpp:89).  Queries that the
restatement flags as ending there are counted and left out: the reference has no defined answer for them.

Golden part (runs everywhere): tests/golden/REF_GP_*.npz hold the O2 build's answers (tests/golden/make_ref_gp_golden.py);
the restatement with its defaults -- the correctly rounded acosf, np.exp -- must reproduce them on bits, from inputs whose
digests match.  tests/test_global_plan_pin_gpu.py holds the device to the cloud cases' goldens."""
import ctypes as C
import ctypes.util
import functools
import math
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
sys.path.insert(0, ROOT)
import global_plan_ref as G  # noqa: E402
import global_plan_cases as Cs  # noqa: E402
import global_plan_pin_cases as P  # noqa: E402
import global_plan_pin_golden as Gd  # noqa: E402
from oracle import ref_gp_py as M  # noqa: E402

F = np.float32
D = np.float64
live = pytest.mark.skipif(not M.available(), reason="oracle/_ref/libref_gp_O0.so / libref_gp_O2.so / ref_gp_asan are absent (no compiled "
                          "reference): run `make -C oracle ref REFERENCE=<checkout>`")
_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.acosf.argtypes, _libm.acosf.restype = [C.c_float], C.c_float


def acosf_libm(c):
    return np.array([_libm.acosf(float(v)) for v in np.asarray(c, F).ravel()], F).reshape(np.shape(c))


def exp_libm(x):
    return np.array([math.exp(float(v)) for v in np.asarray(x, D).ravel()], D).reshape(np.shape(x))


GROUPS = ("hand",) + tuple(f"random-config{i}" for i in range(4)) + tuple(f"cloud-{n}" for n in Gd.CLOUD_CASES)


# ---- the cases and their runs, each computed once ----
@functools.lru_cache(maxsize=None)
def groups() -> dict:
    """group -> {name: case}: the hand-built cases, the random ones by config, the committed queries by cloud case"""
    d = {"hand": {k: v[0] for k, v in P.hand_built().items()}}
    for i, c in enumerate(P.random_cases()):
        d.setdefault(f"random-config{(i // P.QUERIES_PER_GRAPH) % 4}", {})[c["name"]] = c
    for name in Gd.CLOUD_CASES:
        d[f"cloud-{name}"] = {q[0]: P.from_query(q) for q in Cs.queries() if q[1] == name}
    return d


@functools.lru_cache(maxsize=None)
def case_of(name: str) -> dict:
    for g in groups().values():
        if name in g:
            return g[name]
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def libm_run(name: str) -> dict:
    return P.run(case_of(name), exp=exp_libm, acosf=acosf_libm)


@functools.lru_cache(maxsize=None)
def ref_run(name: str, build: str) -> dict:
    return M.plan(case_of(name), build)


def defined(group: str) -> list:
    return [n for n in groups()[group] if not libm_run(n)["ended_on_emptied_set"]]


def bits(a):
    return np.asarray(a, F).view(np.uint32)


def ulps(a, b) -> int:
    """the largest distance in floats between two float32 arrays of non-negative values"""
    a, b = bits(a).astype(np.int64), bits(b).astype(np.int64)
    return int(np.abs(a - b).max()) if len(a) else 0


def against(name: str, build: str, float_ulps: int = 0) -> None:
    """the restatement's libm run against a build: everything discrete equal, g and f within float_ulps floats"""
    r, ref, case = libm_run(name), ref_run(name, build), case_of(name)
    assert (r["status"] == G.FOUND) == (len(ref["path"]) > 0) and r["status"] in (G.FOUND, G.NO_PATH), name
    assert r["path"].tolist() == ref["path"].tolist(), name
    opened = np.flatnonzero(ref["opened"])
    assert sorted(r["g"]) == opened.tolist(), name
    assert [r["parent"][int(i)] for i in opened] == ref["parent"][opened].tolist(), name
    assert sorted(r["closed"]) == np.flatnonzero(ref["closed"]).tolist(), name
    assert r["n_expanded"] == ref["n_closed"] and r["set_size"] == ref["set_size"], (name, r["n_expanded"], ref["n_closed"], r["set_size"], ref["set_size"])
    for k in ("g", "f"):
        mine = np.array([r[k][int(i)] for i in opened], F)
        if float_ulps == 0:
            assert np.array_equal(bits(mine), bits(ref[k][opened])), (name, k)
        else:
            assert ulps(mine, ref[k][opened]) <= float_ulps, (name, k)
    assert len(case["ground"]) == len(ref["opened"])


@functools.lru_cache(maxsize=None)
def measured_gap() -> dict:
    """the reference's own O0-to-O2 gap over every defined case: how many cases differ in anything discrete, and the largest
    distance of an opened node's g or f in floats"""
    gap = dict(cases=0, discrete=0, float_ulps=0, theta_triples=0, theta_differ=0)
    for g in groups():
        for n in defined(g):
            a, b = ref_run(n, "O0"), ref_run(n, "O2")
            gap["cases"] += 1
            same = a["path"].tolist() == b["path"].tolist() and a["set_size"] == b["set_size"] and \
                all(np.array_equal(a[k], b[k]) for k in ("opened", "closed", "parent"))
            gap["discrete"] += not same
            if same:
                o = np.flatnonzero(a["opened"])
                gap["float_ulps"] = max(gap["float_ulps"], ulps(a["g"][o], b["g"][o]), ulps(a["f"][o], b["f"][o]))
    xy = theta_triples()
    gap["theta_triples"] = len(xy)
    gap["theta_differ"] = int((M.theta(xy, "O0").view(np.uint64) != M.theta(xy, "O2").view(np.uint64)).sum())
    return gap


@functools.lru_cache(maxsize=None)
def theta_triples() -> np.ndarray:
    """[n,6] parent, current, expanding x y: random ones at three scales and kilometres out, collinear and reversed ones,
    zero vectors on either side, |vx1| against |vx2| around 0.0001, angles around the cap, and every (parent, current,
    successor) triple of the hand-built fans"""
    rng = np.random.default_rng(77)
    parts = []
    for scale, shift in ((1.0, 0.0), (0.3, 0.0), (0.001, 0.0), (0.5, 4000.0)):
        parts.append((rng.uniform(-1, 1, (22000, 6)) * scale + shift).astype(F))
    p = rng.uniform(-1, 1, (6000, 2))
    v = rng.uniform(-0.5, 0.5, (6000, 2))
    k = rng.uniform(-2, 2, (6000, 1))
    parts.append(np.concatenate([p, p + v, p + v + k * v], axis=1).astype(F))                      # collinear: cosines at and over +-1
    z = (rng.uniform(-1, 1, (1500, 6))).astype(F)
    z[:500, 2:4] = z[:500, 0:2]                                                                  # zero parent vector
    z[500:1000, 4:6] = z[500:1000, 2:4]                                                          # zero expanding vector
    z[1000:, 0:2] = z[1000:, 2:4] = z[1000:, 4:6]                                                # both
    parts.append(z)
    a = np.zeros((4000, 6), F)                                                                   # |vx1| - |vx2| around 0.0001
    a[:, 2] = F(0.0002)
    a[:, 4] = (rng.uniform(0.00009, 0.00011, 4000)).astype(F)
    a[:, 5] = rng.uniform(-0.5, 0.5, 4000)
    for k in range(-3, 4):
        a[k + 3, 4] = G._steps(F(0.0001), k)
    parts.append(a)
    ang = rng.uniform(0.345 - 2e-6, 0.345 + 2e-6, 8000) * rng.choice([-1.0, 1.0], 8000)          # around the cap, both signs
    r = rng.uniform(0.1, 0.5, 8000)
    c = np.zeros((8000, 6), F)
    c[:, 2] = 1.0
    c[:, 4], c[:, 5] = F(1.0) + (r * np.cos(ang)).astype(F), (r * np.sin(ang)).astype(F)
    parts.append(c)
    for name in ("theta-near-cap", "vx-gap-near", "cos-over-one"):
        g = P.hand_built()[name][0]["ground"]
        parts.append(np.array([[g[0, 0], g[0, 1], g[1, 0], g[1, 1], g[i, 0], g[i, 1]] for i in range(2, len(g) - 1)], F))
    return np.concatenate(parts)


# ---- everywhere: the cases hold what they are built for ----
def test_pin_cases_hold_their_conditions():
    found = P.check()
    print(found)
    names = [n for g in groups().values() for n in g]
    assert len(set(names)) == len(names) and tuple(groups()) == GROUPS and tuple(Gd.files()) == Gd.FILES


# ---- the live part ----
@live
def test_theta_on_bits():
    xy = theta_triples()
    assert len(xy) >= 100_000
    mine = G.theta_many(xy, acosf=acosf_libm)
    ref = M.theta(xy, "O0")
    assert not np.isnan(ref).any()
    differ = np.flatnonzero(mine.view(np.uint64) != ref.view(np.uint64))
    assert len(differ) == 0, (len(differ), xy[differ[:3]], mine[differ[:3]], ref[differ[:3]])
    # the correctly rounded acosf is another function: the default restatement differs from the reference somewhere here
    rounded = G.theta_many(xy)
    n = int((rounded.view(np.uint64) != ref.view(np.uint64)).sum())
    print(f"{len(xy)} triples, {int((ref != 0).sum())} with a turn; the correctly rounded acosf differs from libm's on {n}")
    assert n > 0


@live
@pytest.mark.parametrize("group", GROUPS)
def test_group_against_the_O0_build_on_bits(group):
    names = defined(group)
    print(f"{group}: {len(names)} cases compared, {len(groups()[group]) - len(names)} end on the emptied set and are left out")
    assert names
    for n in names:
        against(n, "O0")


@live
def test_O2_build_within_the_references_own_gap():
    gap = measured_gap()
    print(gap)
    assert gap["discrete"] == 0, gap                   # (a finding to look at by hand, should it ever happen)
    for g in groups():
        for n in defined(g):
            against(n, "O2", gap["float_ulps"])
    stored = Gd.load("REF_GP_hand.npz")["gap"]
    assert {k: stored[k] for k in ("discrete", "float_ulps", "theta_differ")} == {k: gap[k] for k in ("discrete", "float_ulps", "theta_differ")}


@live
def test_every_pinned_case_through_the_sanitizer_program():
    names = [n for g in groups() for n in defined(g)]
    left_out = sum(len(g) for g in groups().values()) - len(names)
    assert len(names) >= 800 and all(not libm_run(n)["ended_on_emptied_set"] for n in names)
    with tempfile.TemporaryDirectory() as tmp:
        file = os.path.join(tmp, "cases.bin")
        M.write_cases(file, (case_of(n) for n in names), theta_triples())
        r = subprocess.run([M.ASAN, file], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(names) + 1 and lines[-1].startswith(f"theta {len(theta_triples())} ")
    for n, line in zip(names, lines):                  # the program ran the same searches
        ref = ref_run(n, "O0")
        assert line.split()[1:] == [str(len(ref["path"])), str(ref["set_size"])], (n, line)
    print(f"{len(names)} cases through the sanitizer program, {left_out} left out")


@live
@pytest.mark.parametrize("file", Gd.FILES)
def test_goldens_are_the_O2_builds_answers(file):
    g = Gd.load(file)
    cases = Gd.files()[file]
    for n, want in g["answers"].items():
        assert Gd.differences(Gd.answer_of_reference(cases[n], ref_run(n, "O2")), want) == [], (file, n)


# ---- the golden part ----
@pytest.mark.parametrize("file", Gd.FILES)
def test_restatement_reproduces_the_golden(file):
    g = Gd.load(file)
    cases = Gd.files()[file]
    assert g["answers"] and set(g["answers"]) | set(g["not_golden"]) | set(g["excluded"]) == set(cases)
    for n, want in g["answers"].items():
        case = Gd.inline_case(g["raw"], n) if file == "REF_GP_hand.npz" else cases[n]
        assert Gd.digests(cases[n]) == g["sha256"][n], f"{file}: the inputs of {n} are not the golden's: regenerate (tests/golden/make_ref_gp_golden.py)"
        assert Gd.config_of(cases[n]) == g["config"][n]
        if file.startswith("REF_GP_cloud_"):
            r = Cs.reference(n)
        elif file == "REF_GP_hand.npz":
            r = P.run(case)
        else:
            r = P.restated(n)
        assert not r["ended_on_emptied_set"]
        assert Gd.differences(Gd.answer_of_restatement(r), want) == [], (file, n)


def test_goldens_cover_what_they_must():
    every = {f: Gd.load(f) for f in Gd.files()}
    answers = {n: a for g in every.values() for n, a in g["answers"].items()}
    for q in Cs.queries():
        r = Cs.reference(q[0])
        if r["status"] == G.FOUND:
            assert q[0] in answers, q[0]                # all committed FOUND queries are goldens
        if r["ended_on_emptied_set"]:
            assert q[0] not in answers
    assert sum(Cs.reference(q[0])["status"] == G.FOUND for q in Cs.queries()) == 16
    assert {"start_lone", "start_in_pocket"} <= set(answers) and all(answers[n]["status"] == G.NO_PATH for n in ("start_lone", "start_in_pocket"))
    assert set(every["REF_GP_hand.npz"]["answers"]) == set(P.hand_built())
    rnd = every["REF_GP_random.npz"]
    assert len(rnd["answers"]) >= 700 and sum(a["status"] == G.NO_PATH for a in rnd["answers"].values()) >= 50
    for f, g in every.items():
        assert os.path.getsize(os.path.join(Gd.GOLDEN, f)) < (1 << 20), f
        print(f, len(g["answers"]), "goldens;", len(g["excluded"]), "excluded;", "not golden:", g["not_golden"])
