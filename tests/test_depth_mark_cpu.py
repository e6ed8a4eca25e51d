"""CPU tests of the depth camera's selfMark slice: the committed cases keep their margins in the restatement alone
(tests/helpers/depth_mark_ref.py on an observation built by depth_feed_ref), together they reach every outcome, and the C
header, _capi.py and the C++ mirror declare the two entries alike."""
import collections
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from dddmr_navigation_amd import _capi as K
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import depth_feed_ref as F  # noqa: E402
import depth_mark_cases as cases  # noqa: E402
import depth_mark_ref as M  # noqa: E402

NAMES = [c.name for c in cases.CASES]


@pytest.mark.parametrize("name", NAMES)
def test_every_cluster_of_the_committed_seed_keeps_its_margins(name):
    case, _, obs, frs, most, ground, smap, res = cases.built(name)
    ok, offender = M.margins_kept(res)
    worst = {k: min((cl["margins"][k] for cl in res["clusters"]), default=np.inf) for k in ("ground", "map", "key", "hit")}
    print(f"{name}: {len(obs)} observation points, {res['stats']}, smallest margins {worst}")
    assert ok, offender
    assert len(res["clusters"]) == res["stats"]["n_clusters"]          # no cluster is left out
    assert (len(smap) == 0) == (not case.with_map)


def test_the_cases_reach_every_outcome():
    fates = collections.Counter()
    contested = runs = below = 0
    for name in NAMES:
        case, _, obs, _, _, _, _, res = cases.built(name)
        fates.update(cl["fate"] for cl in res["clusters"])
        if len(obs) > 5:
            below += sum(1 for idx in M.euclidean_clusters(obs, case.tol) if len(idx) < case.min_size)
        vox = collections.Counter(tuple(cl["voxel"]) for cl in res["clusters"] if cl["fate"] == M.ACCEPTED)
        contested += sum(1 for v in vox.values() if v > 1)
        sizes = [cl["size"] for cl in res["clusters"]]
        runs += sum(1 for v in collections.Counter(sizes).values() if v >= 3)
    assert below > 0
    assert all(fates[f] > 0 for f in (M.GROUND, M.STATIC, M.OUTSIDE, M.ACCEPTED)), fates
    assert contested >= 1 and runs >= 1
    assert cases.built("contested_voxels")[0].res == 0.3 and cases.built("contested_voxels")[0].tol == 0.05
    assert cases.built("above_20000")[4] > F.VOXELIZE_ABOVE            # the feed's centroid branch
    assert len(cases.built("few_points")[2]) <= 5 and cases.built("few_points")[7]["stats"]["n_accepted"] == 0
    assert {cases.BY_NAME[n].ratio for n in NAMES} >= {0.0, 0.5, 1.0} and {cases.BY_NAME[n].min_size for n in NAMES} >= {1, 5}


def test_sums_are_sequential_and_sizes_descend():
    res = cases.built("one_camera")[7]
    obs = cases.built("one_camera")[2]
    sizes = [cl["size"] for cl in res["clusters"]]
    assert sizes == sorted(sizes, reverse=True)
    big = M.euclidean_clusters(obs, 0.1)
    idx = max(big, key=len)
    s = np.float32(0.0)
    for v in obs[idx, 0]:
        s = np.float32(s + v)
    cl = next(c for c in res["clusters"] if c["size"] == len(idx))
    assert cl["centroid"][0] == np.float32(s / np.float32(len(idx)))
    assert np.all(np.diff(idx) > 0) and [int(g[0]) for g in big] == sorted(int(g[0]) for g in big)


# ---- the two entries are declared alike in the C header, _capi.py and the C++ mirror ---------------------------------
ENTRIES = ("dddmr_rollout_depth_mark_create", "dddmr_rollout_depth_mark_clusters")


def _split_args(text):
    out, depth, cur = [], 0, ""
    for ch in text:
        if ch in "([":
            depth += 1
        if ch in ")]":
            depth -= 1
        if ch == "," and depth == 0:
            out.append(cur.strip())
            cur = ""
        else:
            cur += ch
    return out + [cur.strip()]


def _ctype_of(param):
    """the ctypes class _capi.py is expected to give a C parameter"""
    p = re.sub(r"\s+", " ", param)
    if "dddmr_rollout_ctx*" in p:
        return C.c_void_p
    if "dddmr_depth_mark_config*" in p:
        return C.POINTER(K.DepthMarkConfig)
    if "dddmr_depth_mark_stats*" in p:
        return C.POINTER(K.DepthMarkStats)
    if p.startswith("const double") and "[7]" in p:
        return C.POINTER(C.c_double)
    if p.startswith("size_t "):
        return C.c_size_t
    if "*" in p or "[" in p:
        return C.c_void_p
    raise AssertionError(p)


def test_header_capi_and_cpp_mirror_declare_the_two_entries_alike():
    header = open(os.path.join(ROOT, "include", "dddmr_rollout.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    mirror = open(os.path.join(ROOT, "include", "dddmr_rollout.hpp")).read()
    lib = K.load_library()
    for name, n_args in zip(ENTRIES, (8, 11)):
        m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", header, flags=re.S)
        assert m, f"{name} is not declared in the header"
        params = _split_args(m.group(1))
        assert len(params) == n_args, params
        assert name in K.EXPORTED_SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is C.c_int
        assert [a for a in fn.argtypes] == [_ctype_of(p) for p in params], name
        calls = re.findall(name + r"\s*\((.*?)\)\s*;", mirror, flags=re.S)
        assert calls, f"{name} is not mirrored in dddmr_rollout.hpp"
        for c in calls:
            assert len(_split_args(c)) == n_args, c
    # struct layouts: field by field against the header, sizes against the compiled library
    for struct, cls, which in (("dddmr_depth_mark_config", K.DepthMarkConfig, 11), ("dddmr_depth_mark_stats", K.DepthMarkStats, 12)):
        body = re.search(r"typedef struct \{([^}]*)\}\s*" + struct + r"\s*;", header).group(1)
        fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if not decl:
                continue
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
        want = {"double": C.c_double, "int32_t": C.c_int32, "uint32_t": C.c_uint32}
        assert [(n, want[t]) for n, t in fields] == [(n, t) for n, t in cls._fields_], struct
        assert C.sizeof(cls) == lib.dddmr_rollout_sizeof(which), struct
