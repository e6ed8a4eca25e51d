"""The device's particle measure (dddmr_navigation_amd.localization.ParticleMeasure) against numbers that came out of
mcl_3dl's own measure(): tests/golden/REF_MCL_*.npz, written by tests/golden/make_ref_mcl_golden.py from the reference
compiled against the stand-ins of oracle/ref/shim/ (its O2 build).  The inputs are rebuilt from the
case generators and must hash to what the goldens were computed from.

Per particle of every case: the quality on bits; terms()' ground count and branch equal to what the reference's debug
lines logged; on the particles whose weight is exactly 1 (a map point at the particle's position, untrusted ground)
terms()' score equal to the reference's likelihood on bits; the likelihood within 2 float ulp (a pos_weight 1 ulp apart,
its double chain going through another libm, times an exact score, rounded once; the reference's own O0 and O2 builds
differ by 0 float ulp of likelihood, the gap the goldens carry is added).

A context holds one particle measure, and a new one replaces the one before it: each case makes its own."""
import os
import sys

import numpy as np
import pytest

from dddmr_navigation_amd import configs, localization
from dddmr_navigation_amd.local_planner import LocalPlanner
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import mcl_measure_golden as G  # noqa: E402

pytestmark = pytest.mark.gpu
WEIGHT_ONE = ("flat-edges-on-map-weight-one", "weight-one-room")


@pytest.fixture(scope="module")
def lp():
    with LocalPlanner([configs.bench_theory("C2")], max_points=200_000) as p:
        yield p


def particle_measure(lp, cfg):
    """(a context holds one particle measure: a new one replaces the one before it, so each case makes its own)"""
    return localization.ParticleMeasure(lp, localization.shipped_config(
        match_dist_min=cfg.match_dist_min, match_dist_flat=cfg.match_dist_flat, radius_of_ground_search=cfg.radius_of_ground_search,
        threshold_for_trusted_ground=cfg.threshold_for_trusted_ground, max_map_points=20000, max_ground_points=20000,
        max_particles=512, max_observation_points=2000, max_ground_neighbours=512))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("file", list(G.FILES))
def test_device_reproduces_the_compiled_reference(lp, file):
    n_weight_one = 0
    for name in G.FILES[file][0]:
        cfg, parts, _, _ = G.load_case(file, name)
        want = G.read(file, name)
        G.check_inputs(file, name, parts, want)
        assert len(parts["states"]) <= 300 and len(parts["flat"]) + len(parts["ls"]) <= 2000 and len(parts["map"]) <= 20000
        pm = particle_measure(lp, cfg)
        pm.set_map(parts["map"], parts["ground"], parts["normals"])
        like, qual = pm.measure(parts["flat"], parts["ls"], parts["states"])
        t = pm.terms(len(like))
        what = f"{file}: {name}"
        np.testing.assert_array_equal(bits(qual), bits(want["quality"]), err_msg=what + ": quality")
        np.testing.assert_array_equal(t["n_ground"], want["trace"][:, 0], err_msg=what + ": ground neighbours")
        np.testing.assert_array_equal(t["healthy"], want["branch"] > 0, err_msg=what + ": branch")
        assert bits(pm.last.quality_min) == bits(want["quality_minmax"][0]) and bits(pm.last.quality_max) == bits(want["quality_minmax"][1]), what
        if name in WEIGHT_ONE:
            assert (t["pos_weight"] == np.float32(1)).all() and not t["healthy"].any(), what
            np.testing.assert_array_equal(bits(t["score"]), bits(want["likelihood"]), err_msg=what + ": score_like at weight 1")
            n_weight_one += len(like)
        ul = G.ulps32(like, want["likelihood"])
        print(f"{what}: {len(like)} particles, {int((ul != 0).sum())} likelihoods not bit-equal (max {int(ul.max())} ulp)")
        assert ul.max() <= 2 + want["gap_like_ulp"], (what, int(ul.argmax()), like[ul.argmax()], want["likelihood"][ul.argmax()])
    if file == "REF_MCL_targeted":
        assert n_weight_one == 22
