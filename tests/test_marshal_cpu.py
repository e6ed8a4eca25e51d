"""CPU tests of dddmr_navigation_amd/_marshal.py: what each helper hands to a C call, with expected values written by
hand.  No library, no context."""
import ctypes as C

import numpy as np
import pytest

from dddmr_navigation_amd import _capi as K, _marshal as M


def _floats_at(p, n):
    return np.frombuffer(C.string_at(p, 4 * n), dtype=np.float32)


@pytest.mark.parametrize("shape,dtype,stride", [((5, 3), np.float32, 12), ((5, 4), np.float32, 16), ((5, 6), np.float32, 24),
                                                ((5, 4), np.float64, 16)])
def test_cloud_strides_and_values(shape, dtype, stride):
    src = (np.arange(shape[0] * shape[1]).reshape(shape) * 0.5 - 3.0).astype(dtype)
    a, p, n, s = M.cloud(src, "cloud")
    assert (n, s) == (5, stride) and a.dtype == np.float32 and a.flags.c_contiguous
    assert isinstance(p, C.c_void_p) and p.value == a.ctypes.data
    want = [0.5 * i - 3.0 for i in range(shape[0] * shape[1])]
    assert _floats_at(p, len(want)).tolist() == want


def test_cloud_views_come_out_contiguous():
    base = np.arange(30, dtype=np.float32).reshape(5, 6)
    a, p, n, s = M.cloud(np.asfortranarray(base), "cloud")
    assert (n, s) == (5, 24) and _floats_at(p, 30).tolist() == list(range(30))
    a, p, n, s = M.cloud(base[:, 1:4], "cloud")                    # a column slice: rows 24 bytes apart in the view
    assert (n, s) == (5, 12) and a.flags.c_contiguous
    assert _floats_at(p, 15).tolist() == [6 * r + c for r in range(5) for c in (1, 2, 3)]


@pytest.mark.parametrize("empty", [np.zeros((0, 3), np.float32), [], np.zeros((0,)), np.zeros((0, 6))])
def test_empty_cloud_is_null_zero_twelve(empty):
    _, p, n, s = M.cloud(empty, "cloud")
    assert p is None and n == 0 and s == 12
    _, p, n, s = M.cloud(empty, "states", cols=7)
    assert p is None and n == 0 and s == 12


def test_cloud_rejects_wrong_shapes():
    with pytest.raises(ValueError, match="scan"):
        M.cloud(np.zeros(3, np.float32), "scan")
    with pytest.raises(ValueError):
        M.cloud(np.zeros((5, 2), np.float32), "scan")
    with pytest.raises(ValueError):
        M.cloud(np.zeros((5, 4), np.float32), "map", cols=3)        # an exact column count
    assert M.cloud(np.zeros((5, 7)), "states", cols=7)[2:] == (5, 28)


def test_pose():
    p = M.pose((1.5, -2.0, 0.25, 0.0, 0.0, 0.6, 0.8))
    assert isinstance(p, C.c_double * 7) and list(p) == [1.5, -2.0, 0.25, 0.0, 0.0, 0.6, 0.8]
    assert list(M.pose(np.arange(7, dtype=np.float32))) == [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0]
    for bad in (range(6), range(8)):
        with pytest.raises(ValueError):
            M.pose(bad)


def test_transform():
    t34 = [[1, 0, 0, 0.5], [0, 1, 0, -1.5], [0, 0, 1, 2.0]]
    for T in (t34, t34 + [[0, 0, 0, 1]], np.asfortranarray(np.array(t34, np.float32))):
        t, p = M.transform(T)
        assert t.shape == (3, 4) and t.dtype == np.float64 and t.flags.c_contiguous
        assert [p[i] for i in range(12)] == [1, 0, 0, 0.5, 0, 1, 0, -1.5, 0, 0, 1, 2.0]
    with pytest.raises(ValueError):
        M.transform(np.zeros((3, 3)))


class _Getter:
    """Stands in for int f(int32 lead, float* a, uint32* b, size_t capacity, size_t* n): writes through its pointers."""

    def __init__(self, count, fail_second=False):
        self.count, self.fail_second, self.calls = count, fail_second, []

    def __call__(self, lead, a, b, capacity, n):
        self.calls.append((lead, a is None, b is None, capacity))
        n._obj.value = self.count
        if a is None:
            return K.OK
        if self.fail_second:
            return K.ERR_HIP
        assert capacity >= self.count
        fa = C.cast(a, C.POINTER(C.c_float))
        ub = C.cast(b, C.POINTER(C.c_uint32))
        for i in range(self.count):
            for j in range(3):
                fa[3 * i + j] = 10 * i + j
            ub[i] = 100 + i
        return K.OK


def _raise(rc):
    if rc != K.OK:
        raise RuntimeError(rc)


@pytest.mark.parametrize("count", [0, 1, 5])
def test_two_call_getter(count):
    f = _Getter(count)
    a, b = M.two_call(lambda *args: f(7, *args), _raise, ((3,), np.float32), ((), np.uint32))
    assert a.shape == (count, 3) and a.dtype == np.float32 and b.shape == (count,) and b.dtype == np.uint32
    assert a.tolist() == [[10.0 * i + j for j in range(3)] for i in range(count)] and b.tolist() == [100 + i for i in range(count)]
    assert f.calls == [(7, True, True, 0), (7, False, False, max(count, 1))]


def test_two_call_getter_passes_ready_arrays_whole():
    f = _Getter(2)
    ring = np.full(4, 9, np.uint32)
    a, b = M.two_call(lambda *args: f(0, *args), _raise, ((3,), np.float32), ring)
    assert a.shape == (2, 3) and b is ring and b.tolist() == [100, 101, 9, 9]
    assert f.calls[0] == (0, True, True, 0)


def test_two_call_getter_raises_through_the_checker():
    f = _Getter(3, fail_second=True)
    with pytest.raises(RuntimeError) as e:
        M.two_call(lambda *args: f(0, *args), _raise, ((3,), np.float32), ((), np.uint32))
    assert e.value.args == (K.ERR_HIP,) and len(f.calls) == 2


def test_fixed_getter():
    def f(buf, n):
        C.memmove(buf, bytes([0, 1, 0, 2, 0][:n]), n)
        return K.OK
    assert M.fixed(f, _raise, 5, np.uint8).tolist() == [0, 1, 0, 2, 0]
    out = M.fixed(f, _raise, 5, np.uint8, as_bool=True)
    assert out.dtype == bool and out.tolist() == [False, True, False, True, False]
    with pytest.raises(RuntimeError):
        M.fixed(lambda buf, n: K.ERR_STATE, _raise, 5, np.float64)


def test_struct_from_defaults():
    c = M.struct_from(K.MclConfig, dict(match_dist_min=0.3, max_particles=16), dict(max_particles=64))
    assert isinstance(c, K.MclConfig) and (c.match_dist_min, c.max_particles, c.max_map_points) == (0.3, 64, 0)
    for bad in ("no_such_field", "reserved"):
        with pytest.raises(KeyError):
            M.struct_from(K.MclConfig, {}, {bad: 1})
    with pytest.raises(KeyError):
        M.struct_from(K.DepthLayerConfig, {}, dict(reserved2=1))


def test_every_config_builder_rejects_unknown_and_reserved_keys():
    from dddmr_navigation_amd import configs, depth_layer, localization, marking
    builders = [marking.shipped_config, depth_layer.shipped_config, localization.shipped_config,
                localization.shipped_observation_config, lambda **kw: configs.dd_simple_shipped(**kw)]
    for build in builders:
        for bad in ("no_such_field", "reserved"):
            with pytest.raises(KeyError):
                build(**{bad: 1})
    assert marking.shipped_config(max_markings=64).max_markings == 64
    assert configs.dd_simple_shipped(sim_time=5.0).sim_time == 5.0
