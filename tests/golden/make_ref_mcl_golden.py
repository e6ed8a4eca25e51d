"""Generates tests/golden/REF_MCL_*.npz from mcl_3dl's own measure(), compiled from a reference checkout
(`make -C oracle ref`, oracle/_ref/libref_mcl_O2.so; see oracle/ref/ref_mcl_driver.cpp), so that the particle-measure
pin travels without the reference: the restatement must reproduce every file (tests/test_mcl_measure_pin_cpu.py) and
the HIP path is held against them (tests/test_mcl_measure_pin_gpu.py).

The files hold the reference's outputs and debug trace, the config, the case name and draw count, and a SHA-256 of
every input; the inputs are rebuilt from tests/helpers/mcl_measure_cases.py and mcl_measure_pin_cases.py (only the small
targeted scenes are stored inline).  The format is described in tests/helpers/mcl_measure_golden.py.  Both builds are
run: the largest O0-to-O2 difference of the reference itself goes into every file (gap_roll_ulp, gap_like_ulp).

Run from the repo root:  python tests/golden/make_ref_mcl_golden.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import mcl_measure_golden as G  # noqa: E402
from oracle import ref_mcl_py as M  # noqa: E402


def run(file, name, build):
    cfg, parts, _, _ = G.load_case(file, name)
    return M.measure(cfg, parts["map"], parts["ground"], parts["normals"], parts["flat"], parts["ls"], parts["states"], build)


def main():
    assert M.available(), "oracle/_ref/libref_mcl_*.so missing: make -C oracle ref REFERENCE=<checkout>"
    results, gap_roll, gap_like, n = {}, 0, 0, 0
    for file, name in G.CASES:
        o0, o2 = run(file, name, "O0"), run(file, name, "O2")
        for k in ("quality", "branch"):
            assert o0[k].tobytes() == o2[k].tobytes(), (file, name, k)
        assert o0["trace"][:, 0].tobytes() == o2["trace"][:, 0].tobytes(), (file, name, "n_ground")
        gap_roll = max(gap_roll, int(G.ulps64(o0["trace"][:, 4], o2["trace"][:, 4]).max()))
        gap_like = max(gap_like, int(G.ulps32(o0["likelihood"], o2["likelihood"]).max()))
        n += len(o2["likelihood"])
        results[(file, name)] = o2
    print(f"{n} particles; the reference's O0 and O2 builds differ by at most {gap_roll} double ulp of roll and "
          f"{gap_like} float ulp of likelihood")
    for file, (names, _, _) in G.FILES.items():
        G.write(file, [results[(file, nm)] for nm in names], gap_roll, gap_like)
        print(f"{file}.npz: {os.path.getsize(os.path.join(G.GOLDEN, file + '.npz'))} bytes")


if __name__ == "__main__":
    main()
