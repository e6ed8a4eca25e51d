"""Argument marshalling shared by the host-side mirrors: pure functions between numpy / Python values and what a
C-ABI call takes.  No library and no context here; `call` is any callable that returns a dddmr_status and `check` is
what raises on one (LocalPlanner._check)."""
from __future__ import annotations

import ctypes as C

import numpy as np

_Pose = C.c_double * 7
_PD = C.POINTER(C.c_double)


def ptr(a: np.ndarray):
    """void* of the array's data; the pointer object keeps the array alive (numpy's data_as holds a reference)."""
    return a.ctypes.data_as(C.c_void_p)


def pose(T):
    """x y z qx qy qz qw -> double[7]"""
    v = [float(x) for x in T]
    if len(v) != 7:
        raise ValueError("a pose is 7 values: x y z qx qy qz qw")
    return _Pose(*v)


def transform(T):
    """A 3x4 (or 4x4) row-major transform -> ([3,4] float64 array, its const double*, which keeps the array alive)."""
    t = np.ascontiguousarray(T, dtype=np.float64)
    if t.shape == (4, 4):
        t = np.ascontiguousarray(t[:3])
    if t.shape != (3, 4):
        raise ValueError("transform: 3x4 (or 4x4) row-major")
    return t, t.ctypes.data_as(_PD)


def cloud(a, name: str, min_cols: int = 3, cols: int = 0):
    """[N, >= min_cols] (cols given: [N, cols]) rows -> (float32 C-contiguous array, pointer, N, stride in bytes).
    Anything without an element is the empty cloud: null pointer, count 0, stride 12
    (every entry point accepts that: cloud_arg_ok() in point_grid_plan.hip.h returns true at a count of 0)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.size == 0:
        return a, None, 0, 12
    if a.ndim != 2 or (a.shape[1] != cols if cols else a.shape[1] < min_cols):
        raise ValueError(f"{name} must be [N, {cols or '>=%d' % min_cols}] float32")
    return a, ptr(a), a.shape[0], a.strides[0]


def two_call(call, check, *outs):
    """The getters that report their count: call(*buffers, capacity, count*) once with null buffers for the count, then with
    max(count, 1) rows.  An entry of outs is (trailing shape, dtype) -> zeros [capacity, *shape], returned cut to the count;
    or a ready array of a size the count does not decide, passed to the second call and returned whole."""
    n = C.c_size_t(0)
    check(call(*[None] * len(outs), 0, C.byref(n)))
    cap = max(n.value, 1)
    bufs = [o if isinstance(o, np.ndarray) else np.zeros((cap,) + tuple(o[0]), o[1]) for o in outs]
    check(call(*[ptr(b) for b in bufs], cap, C.byref(n)))
    return [b if b is o else b[: n.value] for b, o in zip(bufs, outs)]


def fixed(call, check, n: int, dtype, as_bool: bool = False):
    """The getters of a known length: call(buffer, n) -> [n] dtype (as_bool: flags as bool)."""
    out = np.zeros(n, dtype)
    check(call(ptr(out), out.size))
    return out.astype(bool) if as_bool else out


def struct_from(cls, defaults: dict, overrides: dict):
    """cls() with defaults, then overrides, set field by field; KeyError on a key that is no field or a reserved one."""
    fields = {f[0] for f in cls._fields_}
    c = cls()
    for k, v in {**defaults, **overrides}.items():
        if k not in fields or k.startswith("reserved"):
            raise KeyError(k)
        setattr(c, k, v)
    return c
