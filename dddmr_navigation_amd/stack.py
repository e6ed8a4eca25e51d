"""Host-side mirror of the perception stack on top of the C-ABI (dddmr_rollout_stack_*): one
StackedPerception::doClear_then_Mark pass over the device layers of a context, each on its own sensor's observation, the
stacked minimum dGraph (get_min_dGraphValue), the lethal masks (aggregateLethal) and the list of ground nodes that changed
(src/dddmr_perception_3d/src/stacked_perception.cpp:72-126,142-155).  All compute and all state live in the HIP library."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi as K
from . import _marshal as M


class PerceptionStack:
    """The stack of one LocalPlanner context over `marking_layer` (marking.MarkingLayer), `depth_layer`
    (depth_layer.DepthLayer) -- both created on the same ground cloud -- and len(host_layers) host slots; an entry of
    `host_layers` is None (unset) or n_ground + 1 float64 values.  `order` = the plugin order as layer ids
    (_capi.STACK_LIDAR, STACK_DEPTH, STACK_HOST0 + slot); default: lidar, depth, host slots."""

    def __init__(self, lp, marking_layer=None, depth_layer=None, host_layers=(), order=None, max_changes=4096, n_ground=None):
        self._lp = lp
        layers = [l for l in (marking_layer, depth_layer) if l is not None]
        if n_ground is None:
            if not layers:
                raise ValueError("a stack of host layers only needs n_ground")
            n_ground = layers[0].n_ground
        self.n_ground = int(n_ground)
        if order is None:
            order = ([K.STACK_LIDAR] if marking_layer is not None else []) + ([K.STACK_DEPTH] if depth_layer is not None else []) + \
                    [K.STACK_HOST0 + i for i in range(len(host_layers))]
        self.order = tuple(int(o) for o in order)
        cfg = K.StackConfig()
        cfg.n_ground = self.n_ground
        cfg.use_lidar_layer = int(marking_layer is not None)
        cfg.use_depth_layer = int(depth_layer is not None)
        cfg.n_host_layers = len(host_layers)
        cfg.n_order = len(self.order)
        for i, o in enumerate(self.order[: K.STACK_MAX_LAYERS]):
            cfg.layer_order[i] = o
        cfg.max_changes = max_changes
        self.cfg = cfg
        lp._call("stack_create", C.byref(cfg))
        for slot, values in enumerate(host_layers):
            if values is not None:
                self.set_host_layer(slot, values)
        self.last = None
        self.totals = dict(updates=0, changed=0, launches=0, host_waits=0, depth_skipped=0)

    def set_host_layer(self, slot: int, values):
        """A layer whose dGraph the host computes (static layer, zone layers): n_ground + 1 float64, None unsets the slot."""
        if values is None:
            self._lp._call("stack_set_host_layer", slot, None)
            return
        v = np.ascontiguousarray(values, dtype=np.float64)
        if v.shape != (self.n_ground + 1,):
            raise ValueError("a host layer is n_ground + 1 float64 values")
        self._lp._call("stack_set_host_layer", slot, M.ptr(v))

    def update(self, T_base_sensor=None, T_gbl_base=None) -> K.StackStats:
        """One pass; raises RolloutError with the first failing layer's code, self.last holds the stats either way."""
        tbs = M.pose(T_base_sensor) if T_base_sensor is not None else None
        tgb = M.pose(T_gbl_base) if T_gbl_base is not None else None
        st = K.StackStats()
        rc = self._lp._rc("stack_update", tbs, tgb, C.byref(st))
        self.last = st
        t = self.totals
        t["updates"] += 1; t["changed"] += st.n_changed; t["launches"] += st.launches; t["host_waits"] += st.host_waits
        t["depth_skipped"] += st.depth_skipped
        self._lp._check(rc)
        return st

    def n_changes(self) -> int:
        """The true count of the last update, also when it exceeds max_changes."""
        n = C.c_size_t(0)
        rc = self._lp._rc("stack_get_changes", None, None, None, 0, C.byref(n))
        if rc != K.ERR_CAPACITY:
            self._lp._check(rc)
        return int(n.value)

    def changes(self):
        """-> (nodes [n] uint32, values [n] float64, masks [n] uint8) of the last update; RolloutError(ERR_CAPACITY) when
        the list overflowed: min_dgraph() / lethal_mask() resynchronise."""
        cap = max(int(self.cfg.max_changes), 1)
        node, value, mask = np.zeros(cap, np.uint32), np.zeros(cap, np.float64), np.zeros(cap, np.uint8)
        n = C.c_size_t(0)
        self._lp._call("stack_get_changes", M.ptr(node), M.ptr(value), M.ptr(mask), cap, C.byref(n))
        return node[: n.value], value[: n.value], mask[: n.value]

    def min_dgraph(self) -> np.ndarray:
        return self._lp._fixed("stack_get_min_dgraph", self.n_ground + 1, np.float64)

    def lethal_mask(self) -> np.ndarray:
        """one byte per node; bit i = the layer at position i of `order`"""
        return self._lp._fixed("stack_get_lethal_mask", self.n_ground + 1, np.uint8)

    def lethal_nodes(self) -> np.ndarray:
        """aggregateLethal as node indices: per device layer in plugin order, its lethal nodes ascending"""
        return self._lp._get("stack_get_lethal_nodes", (), ((), np.uint32))[0]

    def reset(self):
        """StackedPerception::resetdGraph: both layers, then the stacked arrays; the change list is empty afterwards"""
        self._lp._call("stack_reset")

    def summary(self) -> dict:
        t = self.totals
        n = max(t["updates"], 1)
        return {"updates": t["updates"], "changed_per_update": round(t["changed"] / n, 1), "launches_per_update": round(t["launches"] / n, 1),
                "host_waits_per_update": round(t["host_waits"] / n, 2), "depth_skipped": t["depth_skipped"]}

    def close(self):
        pass      # the context owns the device state
