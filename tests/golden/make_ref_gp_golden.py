"""Writes tests/golden/REF_GP_*.npz from the reference's own planner, O2 build (oracle/_ref/libref_gp_O2.so, made by
`make -C oracle ref` from a reference checkout; see oracle/ref/ref_gp_driver.cpp and tests/helpers/global_plan_pin_golden.py
for what a file holds).  Run from the repository root: python tests/golden/make_ref_gp_golden.py

A query becomes a golden when (1) the restatement does not flag it as ending on a set emptied by discards -- the reference
has no defined answer there, and such a query is never sent to it -- and (2) the restatement with its defaults (the
correctly rounded acosf, np.exp) reproduces the O2 build's answer on bits.  The reference's theta is libm's acosf, which
differs from the correctly rounded value in the last bit for about 7 % of arguments, so (2) can fail for a query that the
live pin (libm's acosf on both sides) passes: such queries are listed by name below and in the file, not stored.  The
measured O0-to-O2 gap of the reference over all defined cases is stored in every file."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
sys.path.insert(0, ROOT)
import global_plan_pin_cases as P  # noqa: E402
import global_plan_pin_golden as Gd  # noqa: E402
from oracle import ref_gp_py as M  # noqa: E402


def gap_of(cases) -> dict:
    """the reference's own O0-to-O2 gap over the defined cases (the same measure as tests/test_global_plan_pin_cpu.py's)"""
    gap = dict(cases=0, discrete=0, float_ulps=0)
    for c in cases:
        a, b = M.plan(c, "O0"), M.plan(c, "O2")
        gap["cases"] += 1
        same = a["path"].tolist() == b["path"].tolist() and a["set_size"] == b["set_size"] and \
            all(np.array_equal(a[k], b[k]) for k in ("opened", "closed", "parent"))
        gap["discrete"] += not same
        if same:
            o = np.flatnonzero(a["opened"])
            for k in ("g", "f"):
                d = np.abs(a[k][o].view(np.uint32).astype(np.int64) - b[k][o].view(np.uint32).astype(np.int64))
                gap["float_ulps"] = max(gap["float_ulps"], int(d.max()) if len(d) else 0)
    return gap


def main():
    assert M.available(), "oracle/_ref/libref_gp_*.so are absent: make -C oracle ref"
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_global_plan_pin_cpu as T                                       # the theta triples of the live pin
    xy = T.theta_triples()
    theta_differ = int((M.theta(xy, "O0").view(np.uint64) != M.theta(xy, "O2").view(np.uint64)).sum())
    runs, defined = {}, []
    for file, cases in Gd.files().items():
        for n, c in cases.items():
            runs[n] = P.run(c)
            if not runs[n]["ended_on_emptied_set"]:
                defined.append(c)
    gap = gap_of(defined)
    gap.update(theta_triples=len(xy), theta_differ=theta_differ)
    print("O0-to-O2 gap:", gap)
    for file, cases in Gd.files().items():
        names, kept, answers, not_golden, excluded = [], [], [], {}, []
        for n, c in cases.items():
            if runs[n]["ended_on_emptied_set"]:
                excluded.append(n)
                continue
            want = Gd.answer_of_reference(c, M.plan(c, "O2"))
            diff = Gd.differences(Gd.answer_of_restatement(runs[n]), want)
            if diff:
                not_golden[n] = "the restatement's defaults differ in " + ", ".join(diff)
                continue
            names.append(n)
            kept.append(c)
            answers.append(want)
        np.savez_compressed(os.path.join(Gd.GOLDEN, file), **Gd.pack(names, kept, answers, gap, not_golden, excluded, inline=file == "REF_GP_hand.npz"))
        print(f"{file}: {len(names)} goldens, {len(excluded)} end on the emptied set, {os.path.getsize(os.path.join(Gd.GOLDEN, file))} bytes")
        for n, why in not_golden.items():
            print(f"  not a golden: {n}: {why}")


if __name__ == "__main__":
    main()
