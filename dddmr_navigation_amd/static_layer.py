"""Host-side mirror of the static layer and the no-entry layer on top of the C-ABI (dddmr_rollout_static_layer_*):
StaticLayer::selfClear's regeneration (dddmr_perception_3d/plugins/static_layer.cpp:201-285, :390-415) -- sGraph as CSR
rows and the layer's dGraph -- and the zones' inflation (no_entry_layer.cpp:265-283).  All compute and all state live in
the HIP library; a dGraph reaches the perception stack device to device (bind)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi as K
from . import _marshal as M


def shipped_config(**kw) -> K.StaticLayerConfig:
    """p2p_move_base_localization.yaml's static layer, with room for a 100 000-node ground."""
    return M.struct_from(K.StaticLayerConfig, dict(
        max_ground_points=1 << 17, max_map_points=1 << 18, max_edges=1 << 24, use_adaptive_connection=0, adaptive_connection_number=20,
        radius_of_ground_connection=1.5, static_imposing_radius=1.5, inscribed_radius=0.5, max_obstacle_distance=9999.0,
        enable_edge_detection=1, generate_static_graph=1), kw)


class StaticLayer:
    """The static layer's graphs of one context.  `last` keeps the stats of the latest build or set_zones, also when the
    call raises (a build beyond max_edges reports the true edge count there)."""

    def __init__(self, lp, cfg: K.StaticLayerConfig):
        self._lp = lp
        self.cfg = cfg
        lp._call("static_layer_create", C.byref(cfg))
        self.last = None
        self.n_ground = 0

    def build(self, ground_xyz, map_xyz) -> K.StaticLayerStats:
        """One regeneration from the ground [G,3+] and map [M,3+] clouds (only x y z are read)."""
        _, gp, gn, gs = M.cloud(ground_xyz, "ground")
        _, mp, mn, ms = M.cloud(map_xyz, "map")
        st = K.StaticLayerStats()
        rc = self._lp._rc("static_layer_build", gp, gn, gs, mp, mn, ms, C.byref(st))
        self.last = st
        self._lp._check(rc)
        self.n_ground = int(st.n_ground)
        return st

    def stats(self):
        return self.last

    def graph(self) -> dict:
        """sGraph as CSR: row_start [n_ground + 1] uint32, neighbour [n_edges] uint32 (ascending in a row), weight float32."""
        n = C.c_size_t(0)
        self._lp._call("static_layer_get_graph", None, None, None, 0, C.byref(n))
        cap = max(n.value, 1)
        rs, nb, w = np.zeros(self.n_ground + 1, np.uint32), np.zeros(cap, np.uint32), np.zeros(cap, np.float32)
        self._lp._call("static_layer_get_graph", M.ptr(rs), M.ptr(nb), M.ptr(w), cap, C.byref(n))
        return dict(row_start=rs, neighbour=nb[: n.value], weight=w[: n.value])

    def dgraph(self) -> np.ndarray:
        """The static layer's dGraph: n_ground + 1 doubles."""
        return M.fixed(lambda *a: self._lp._rc("static_layer_get_dgraph", *a), self._lp._check, self.n_ground + 1, np.float64)

    def set_zones(self, zone_xyz, inflation_distance: float) -> K.StaticLayerStats:
        """The enabled zones' points [Z,3+], concatenated (none: every zone is off) -> the no-entry dGraph is rebuilt."""
        _, zp, zn, zs = M.cloud(zone_xyz, "zones")
        st = K.StaticLayerStats()
        rc = self._lp._rc("static_layer_set_zones", zp, zn, zs, float(inflation_distance), C.byref(st))
        self.last = st
        self._lp._check(rc)
        return st

    def zone_dgraph(self) -> np.ndarray:
        return M.fixed(lambda *a: self._lp._rc("static_layer_get_zone_dgraph", *a), self._lp._check, self.n_ground + 1, np.float64)

    def bind(self, which: int, slot: int):
        """which 0: the static dGraph, 1: the no-entry dGraph -> host slot `slot` of the context's perception stack."""
        self._lp._call("static_layer_bind", int(which), int(slot))

    def close(self):
        pass      # the context owns the device state
