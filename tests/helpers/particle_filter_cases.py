"""Inputs of the particle filter tests (tests/test_particle_filter_cpu.py, tests/test_particle_filter_gpu.py): particle
sets, probability and likelihood cases, noise rows.  Everything is a function of (n, a name) alone."""
import os

import numpy as np

import particle_filter_ref as R

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden")
GOLDEN_SIZES = (1, 2, 16, 17, 60, 257)
# one, two, around a wave, more than one workgroup of the per-particle kernels (256), more than one staged chunk of the
# serial loops (2048)
SIZES = (1, 2, 63, 64, 65, 257, 1000, 4096)
U_MAX = np.nextafter(F(1), F(0))
LIN_TC, ANG_TC, VAR_DIST, VAR_ANG = 5.0, 10.0, 2.0, 1.57
STATE_PREV = np.array([3.1, -2.05, 0.52, 0.0, 0.005, 0.19866933, 0.98006658], F)
ODOM_PREV = np.array([10.0, 4.0, 0.1, 0.0, 0.0, 0.34289781, 0.93937271], F)
ODOM_CUR = np.array([10.12, 4.09, 0.11, 0.001, -0.002, 0.36161551, 0.93232695], F)
DT = 0.1


def golden(n: int) -> dict:
    return dict(np.load(os.path.join(GOLDEN, f"REF_MCL_PF_N{n}.npz")))


def particles(n: int, seed: int = 0):
    """-> (states [n,13], noise4 [n,4]): poses around (3, -2, 0.5), any yaw, small roll / pitch, used integrals"""
    rng = np.random.default_rng(1000 + 7 * n + seed)
    s = np.zeros((n, 13), F)
    s[:, 0:3] = np.array([3.0, -2.0, 0.5], F) + rng.uniform(-1, 1, (n, 3)).astype(F) * np.array([1, 1, 0.2], F)
    rpy = rng.uniform(-1, 1, (n, 3)).astype(F) * np.array([0.1, 0.1, 3.1], F)
    s[:, 3:7] = np.stack([R.quat_from_rpy(r) for r in rpy])
    s[:, 7:13] = rng.uniform(-0.05, 0.05, (n, 6)).astype(F)
    z = (rng.uniform(-1, 1, (n, 4)) * np.array([0.6, 0.3, 0.3, 0.6])).astype(F)
    return s, z


def probability(n: int, kind: str):
    """normalised: uneven weights that sum to 1;  sum1.5: the same times 1.5, so that expectation(1.0)'s break falls inside
    the array (for n > 1)"""
    rng = np.random.default_rng(100 + n)
    p = rng.uniform(0.2, 1.0, n).astype(F)
    p = (p / p.sum(dtype=F)).astype(F)
    return {"normalised": p, "sum1.5": (p * F(1.5)).astype(F)}[kind]


LIKELIHOODS = ("plain", "third-zero", "all-zero", "tiny")


def likelihood(n: int, kind: str):
    """plain: in [0.05, 1];  third-zero: every third one 0 (equal neighbours in accum);  all-zero: pf::measure restores;
    tiny: 1e-12 beside values near 1 (adds the running sum absorbs)"""
    rng = np.random.default_rng(300 + n)
    lk = rng.uniform(0.05, 1.0, n).astype(F)
    if kind == "third-zero":
        lk[::3] = 0
        if n == 1:
            lk[0] = F(0.5)
    elif kind == "all-zero":
        lk[:] = 0
    elif kind == "tiny":
        lk[:] = rng.uniform(0.9, 1.0, n).astype(F)
        lk[1::2] = F(1e-12)
    return lk


def noise_rows(n: int, seed: int = 0):
    """[n,10] rows as generateNoise builds them from six draws of sigma (0.2 0.2 0.2 | 0.2 0.2 0.1)"""
    rng = np.random.default_rng(500 + n + seed)
    d = (rng.standard_normal((n, 6)) * np.array([0.2, 0.2, 0.2, 0.2, 0.2, 0.1])).astype(F)
    return np.stack([R.noise_row(r) for r in d]).astype(F)
