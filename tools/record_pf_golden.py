#!/usr/bin/env python3
"""Builds tools/record_pf_golden.cpp against a checkout of the reference (its include/mcl_3dl headers, the stand-ins of
oracle/ref/shim, the flags oracle/Makefile pins the reference with) and writes tests/golden/REF_MCL_PF_N<n>.npz: the inputs,
the engine's draws and the particle set after each stage as mcl_3dl's own pf.h / state_6dof.h / motion model answer.
No test runs this; the goldens are committed.

    python tools/record_pf_golden.py --reference /path/to/reference [--out tests/golden]
"""
import argparse
import os
import shutil
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 2, 16, 17, 60, 257)
SEED = 20240521
FLAGS = ["-O2", "-march=x86-64", "-ffp-contract=off", "-fno-fast-math", "-std=c++17", "-w"]
LIMIT = 1 << 20          # a committed file's size limit


def parse(path: str) -> dict:
    out, raw, at = {}, open(path, "rb").read(), 0
    while at < len(raw):
        (ln,) = struct.unpack_from("<I", raw, at)
        name = raw[at + 4: at + 4 + ln].decode()
        at += 4 + ln
        kind = chr(raw[at])
        (rank,) = struct.unpack_from("<I", raw, at + 1)
        dims = struct.unpack_from(f"<{rank}I", raw, at + 5)
        at += 5 + 4 * rank
        count = int(np.prod(dims))
        out[name] = np.frombuffer(raw, dtype=np.float32 if kind == "f" else np.uint32, count=count, offset=at).reshape(dims).copy()
        at += 4 * count
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    cxx = shutil.which("g++") or shutil.which("c++")
    inc = os.path.join(a.reference, "src", "dddmr_mcl_3dl", "include")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "record_pf_golden")
        subprocess.run([cxx, *FLAGS, "-I", os.path.join(ROOT, "oracle", "ref", "shim"),
                        "-I", os.path.join(ROOT, "tools", "record_pf_shim"), "-I", inc,
                        os.path.join(ROOT, "tools", "record_pf_golden.cpp"), "-o", exe], check=True)
        for n in SIZES:
            raw = os.path.join(tmp, f"n{n}.bin")
            subprocess.run([exe, str(n), str(SEED + n), raw], check=True)
            rec = parse(raw)
            assert int(rec["n"][0]) == n and (n <= 16 or int(rec["resample_ties"][0]) == 0), n
            dst = os.path.join(a.out, f"REF_MCL_PF_N{n}.npz")
            np.savez_compressed(dst, **rec)
            size = os.path.getsize(dst)
            assert size < LIMIT, (dst, size)
            print(f"{dst}: {len(rec)} arrays, {size} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
