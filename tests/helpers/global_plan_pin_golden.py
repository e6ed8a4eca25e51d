"""The planner pin's goldens (tests/golden/REF_GP_*.npz): what a file holds, how a case's inputs are digested and how an
answer is compared with a stored one.  Shared by tests/golden/make_ref_gp_golden.py (which writes them from the reference's
O2 build), tests/test_global_plan_pin_cpu.py (the restatement must reproduce them on bits) and
tests/test_global_plan_pin_gpu.py (the device, on the cloud cases).

A file holds, for queries 0..n-1: name, status, path (path_start[n+1] into path_nodes), the records of the path's nodes
(path_g, path_f, path_parent, aligned with path_nodes), g_goal, n_closed (the closed count: n_expanded), set_size (the
final size of the reference's set), config (JSON), sha256 (JSON: one digest per input), and once: gap (JSON: the measured
O0-to-O2 gap of the reference), not_golden (the names the generator left out, with the reason) and excluded (the names
whose search ends on the emptied set).  REF_GP_hand.npz also holds every hand-built case's inputs inline under
"<name>/<input>"; the other files' inputs are rebuilt from their generators and checked against the digests."""
from __future__ import annotations

import functools
import hashlib
import json
import os

import numpy as np

import global_plan_cases as Cs
import global_plan_pin_cases as P
import global_plan_ref as G

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(os.path.dirname(HERE), "golden")
CLOUD_CASES = ("floor", "floor_shifted", "long_row", "lattice")
INPUTS = (("ground", np.float32), ("intensity", np.float32), ("row_start", np.uint32), ("neighbour", np.uint32), ("weight", np.float32),
          ("order", np.uint32), ("dgraph", np.float64))
CFG_KEYS = ("turning_weight", "a_star_expanding_radius", "inscribed_radius", "inflation_descending_rate")


FILES = ("REF_GP_hand.npz", "REF_GP_random.npz") + tuple(f"REF_GP_cloud_{n}.npz" for n in CLOUD_CASES)


@functools.lru_cache(maxsize=None)
def files() -> dict:
    """file name -> the pin cases it covers, by name (excluded and not-golden ones included)"""
    d = {"REF_GP_hand.npz": {k: v[0] for k, v in P.hand_built().items()}, "REF_GP_random.npz": {c["name"]: c for c in P.random_cases()}}
    for name in CLOUD_CASES:
        d[f"REF_GP_cloud_{name}.npz"] = {q[0]: P.from_query(q) for q in Cs.queries() if q[1] == name}
    return d


def inputs(case: dict) -> dict:
    out = {}
    for k, t in INPUTS:
        v = case.get(k)
        out[k] = np.zeros(0, t) if v is None else np.ascontiguousarray(v, t)
    return out


def config_of(case: dict) -> str:
    d = {k: float(case["cfg"][k]) for k in CFG_KEYS}
    d.update(start=int(case["start"]), goal=int(case["goal"]))
    return json.dumps(d, sort_keys=True)


def digests(case: dict) -> str:
    d = {k: hashlib.sha256(v.tobytes()).hexdigest() for k, v in inputs(case).items()}
    d["config"] = hashlib.sha256(config_of(case).encode()).hexdigest()
    return json.dumps(d, sort_keys=True)


def answer_of_reference(case: dict, ref: dict) -> dict:
    """what a golden keeps of one getPath of the reference (oracle/ref_gp_py.plan)"""
    path = ref["path"].astype(np.uint32)
    found = len(path) > 0
    return dict(status=G.FOUND if found else G.NO_PATH, path=path, path_g=ref["g"][path], path_f=ref["f"][path], path_parent=ref["parent"][path],
                g_goal=F(ref["g"][case["goal"]]) if found else F(0), n_closed=int(ref["n_closed"]), set_size=int(ref["set_size"]))


def answer_of_restatement(r: dict) -> dict:
    path = r["path"].astype(np.uint32)
    return dict(status=int(r["status"]), path=path, path_g=np.array([r["g"][int(i)] for i in path], F), path_f=np.array([r["f"][int(i)] for i in path], F),
                path_parent=np.array([r["parent"][int(i)] for i in path], np.uint32), g_goal=F(r["g_goal"]), n_closed=int(r["n_expanded"]),
                set_size=int(r["set_size"]))


def differences(a: dict, b: dict) -> list:
    """the fields in which two answers differ, on bits"""
    out = []
    for k in ("status", "n_closed", "set_size"):
        if int(a[k]) != int(b[k]):
            out.append(k)
    for k, t in (("path", np.uint32), ("path_parent", np.uint32), ("path_g", np.uint32), ("path_f", np.uint32)):
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.shape != y.shape or not np.array_equal(x.view(t) if x.dtype == F else x, y.view(t) if y.dtype == F else y):
            out.append(k)
    if F(a["g_goal"]).view(np.uint32) != F(b["g_goal"]).view(np.uint32):
        out.append("g_goal")
    return out


def pack(names, cases, answers, gap, not_golden, excluded, inline=False) -> dict:
    d = dict(name=np.array(names), status=np.array([a["status"] for a in answers], np.int32),
             path_start=np.concatenate([[0], np.cumsum([len(a["path"]) for a in answers])]).astype(np.int64),
             g_goal=np.array([a["g_goal"] for a in answers], F), n_closed=np.array([a["n_closed"] for a in answers], np.int64),
             set_size=np.array([a["set_size"] for a in answers], np.int64), config=np.array([config_of(c) for c in cases]),
             sha256=np.array([digests(c) for c in cases]), gap=np.array(json.dumps(gap, sort_keys=True)),
             not_golden=np.array(json.dumps(not_golden, sort_keys=True)), excluded=np.array(sorted(excluded)))
    for k, t in (("path", np.uint32), ("path_g", F), ("path_f", F), ("path_parent", np.uint32)):
        parts = [np.asarray(a[k], t) for a in answers]
        d["path_nodes" if k == "path" else k] = np.concatenate(parts) if parts else np.zeros(0, t)
    if inline:
        for n, c in zip(names, cases):
            for k, v in inputs(c).items():
                d[f"{n}/{k}"] = v
    return d


def load(file: str) -> dict:
    """file name -> dict(answers: name -> answer, config, sha256, gap, not_golden, excluded, raw: the npz)"""
    z = np.load(os.path.join(GOLDEN, file), allow_pickle=False)
    out = dict(answers={}, config={}, sha256={}, gap=json.loads(str(z["gap"])), not_golden=json.loads(str(z["not_golden"])),
               excluded=[str(x) for x in z["excluded"]], raw=z)
    ps = z["path_start"]
    for i, n in enumerate(str(x) for x in z["name"]):
        s = slice(int(ps[i]), int(ps[i + 1]))
        out["answers"][n] = dict(status=int(z["status"][i]), path=z["path_nodes"][s], path_g=z["path_g"][s], path_f=z["path_f"][s],
                                 path_parent=z["path_parent"][s], g_goal=F(z["g_goal"][i]), n_closed=int(z["n_closed"][i]), set_size=int(z["set_size"][i]))
        out["config"][n] = str(z["config"][i])
        out["sha256"][n] = str(z["sha256"][i])
    return out


def inline_case(z, name: str) -> dict:
    """a hand-built case from the inputs stored in REF_GP_hand.npz (the config from its JSON)"""
    i = [str(x) for x in z["name"]].index(name)
    cfg = json.loads(str(z["config"][i]))
    c = {k: z[f"{name}/{k}"] for k, _ in INPUTS}
    c["ground"] = c["ground"].reshape(-1, 3)
    if len(c["intensity"]) == 0:
        c["intensity"] = None
    c.update(name=name, start=cfg.pop("start"), goal=cfg.pop("goal"), cfg=G.config(**cfg))
    return c
