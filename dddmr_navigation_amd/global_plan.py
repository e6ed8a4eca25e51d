"""Host-side mirror of the pre-graph global planner on top of the C-ABI (dddmr_rollout_global_plan_*):
A_Star_on_PreGraph::getPath (dddmr_global_planner/src/a_star_on_pre_graph.cpp:191-289) over the static layer's sGraph and a
dGraph that is already on the device, getStartGoalID's nearest-node search (global_planner.cpp:407, :451) and
determineDWAPlan's goal test (dynamic_window_aware_global_planner.cpp:248-270); and of the default planner,
A_Star_on_Graph::getPath with isLineOfSightClear (a_star_on_pc.cpp:168-329), on the ground cloud itself.  All compute and all state live in the HIP
library; a plan returns node ids of the static layer's ground cloud."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _capi as K
from . import _marshal as M


def shipped_config(**kw) -> K.GlobalPlanConfig:
    """global_planner's shipped parameters (turning_weight 0.1, a_star_expanding_radius 0.5) with perception's inscribed_radius
    and inflation_descending_rate, the stack's dGraph, and room for a 100 000-node ground."""
    return M.struct_from(K.GlobalPlanConfig, dict(
        turning_weight=0.1, a_star_expanding_radius=0.5, inscribed_radius=0.5, inflation_descending_rate=2.0, dgraph_source=0,
        max_queries=K.GLOBAL_PLAN_MAX_QUERIES, max_open_entries=1 << 20, max_expansions=1 << 17), kw)


@dataclass
class Plan:
    status: int
    path: np.ndarray            # uint32 node ids from start to goal; empty unless status is GLOBAL_PLAN_FOUND
    n_expanded: int
    n_pushed: int
    n_discarded_closed: int
    g_goal: np.float32
    host_waits: int


@dataclass
class CloudPlan(Plan):
    """A plan of plan_on_cloud: Plan's fields, then what the search met on its way."""
    n_knn_fallbacks: int        # expansions that took the 8 nearest nodes (fewer than 8 inside the radius)
    n_lethal_skipped: int       # successors below inscribed_radius
    n_los_tested: int           # edges of 2 * inscribed_radius or more: marched
    n_los_blocked: int          # ... and refused by the march
    n_los_capped: int           # ... of these, by the sample cap
    max_successors: int         # the longest successor list


class GlobalPlan:
    """The global planner of one context; needs a StaticLayer of the same context (and a PerceptionStack for dgraph_source 0).
    A context has one planner: creating another GlobalPlan on it replaces the first one's device state and parameters.
    `last_results` keeps the results of the latest plan call, also when it raises (OPEN_FULL)."""

    def __init__(self, lp, cfg: K.GlobalPlanConfig, max_nodes: int):
        self._lp = lp
        self.cfg = cfg
        self.max_nodes = int(max_nodes)          # the static layer's max_ground_points: the longest path
        lp._call("global_plan_create", C.byref(cfg))
        self.last_results = None

    def set_node_weights(self, weights):
        """The ground cloud's intensity, one per ground node (None or empty: all zero)."""
        w = np.ascontiguousarray(np.zeros(0) if weights is None else weights, dtype=np.float32).ravel()
        self._lp._call("global_plan_set_node_weights", M.ptr(w) if w.size else None, w.size)

    def _points(self, xyz):
        p = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        return p, (M.ptr(p) if len(p) else None)

    def nearest(self, xyz) -> np.ndarray:
        """[N,3] points -> [N] uint32 node ids, K.GLOBAL_PLAN_NONE without a ground node inside 0.5 m."""
        p, pp = self._points(xyz)
        ids = np.full(len(p), K.GLOBAL_PLAN_NONE, np.uint32)
        self._lp._call("global_plan_nearest", pp, len(p), M.ptr(ids) if len(p) else None)
        return ids

    def probe(self, xyz):
        """[N,3] points -> ([N] uint32 ground nodes inside 0.25 m, [N] bool: one of them is below inscribed_radius)."""
        p, pp = self._points(xyz)
        cnt, blocked = np.zeros(len(p), np.uint32), np.zeros(len(p), np.uint8)
        self._lp._call("global_plan_probe", pp, len(p), M.ptr(cnt) if len(p) else None, M.ptr(blocked) if len(p) else None)
        return cnt, blocked.astype(bool)

    def plan_many(self, starts, goals, path_capacity: int = 0) -> list:
        """Independent searches in one launch (at most cfg.max_queries) -> a Plan per query."""
        s = np.ascontiguousarray(starts, dtype=np.uint32).ravel()
        g = np.ascontiguousarray(goals, dtype=np.uint32).ravel()
        if s.size != g.size or s.size == 0:
            raise ValueError("as many starts as goals, at least one")
        cap = int(path_capacity) or s.size * self.max_nodes
        path = np.zeros(max(cap, 1), np.uint32)
        res = (K.GlobalPlanResult * s.size)()
        rc = self._lp._rc("global_plan_plan", M.ptr(s), M.ptr(g), s.size, M.ptr(path), cap, res)
        self.last_results = list(res)
        self._lp._check(rc)
        return [Plan(int(r.status), path[r.path_offset: r.path_offset + r.path_len].copy(), int(r.n_expanded), int(r.n_pushed),
                     int(r.n_discarded_closed), np.float32(r.g_goal), int(r.host_waits)) for r in res]

    def plan(self, start: int, goal: int) -> Plan:
        return self.plan_many([start], [goal])[0]

    # ---- the default A* on the ground cloud (A_Star_on_Graph::getPath, a_star_on_pc.cpp:200-329) ----
    def set_graph_node_weights(self, weights):
        """sGraph's node weights (static_graph.cpp:62, added at a_star_on_pc.cpp:288), one per ground node (None or empty:
        all zero).  A second array beside set_node_weights' intensity."""
        w = np.ascontiguousarray(np.zeros(0) if weights is None else weights, dtype=np.float32).ravel()
        self._lp._call("global_plan_set_graph_node_weights", M.ptr(w) if w.size else None, w.size)

    def set_lethal_points(self, xyz):
        """The lethal points of the layers left on the host, [N,3] (None or empty: none); a duplicate is two points."""
        p, pp = self._points(np.zeros((0, 3)) if xyz is None else xyz)
        self._lp._call("global_plan_set_lethal_points", pp, len(p), 12)

    def plan_many_on_cloud(self, starts, goals, path_capacity: int = 0) -> list:
        """plan_many with A_Star_on_Graph::getPath: radius-search successors, line of sight against the lethal cloud -> a
        CloudPlan per query.  `last_results` keeps the raw results, also when the call raises (OPEN_FULL, ROW_FULL)."""
        s = np.ascontiguousarray(starts, dtype=np.uint32).ravel()
        g = np.ascontiguousarray(goals, dtype=np.uint32).ravel()
        if s.size != g.size or s.size == 0:
            raise ValueError("as many starts as goals, at least one")
        cap = int(path_capacity) or s.size * self.max_nodes
        path = np.zeros(max(cap, 1), np.uint32)
        res = (K.GlobalPlanCloudResult * s.size)()
        rc = self._lp._rc("global_plan_plan_on_cloud", M.ptr(s), M.ptr(g), s.size, M.ptr(path), cap, res)
        self.last_results = list(res)
        self._lp._check(rc)
        return [CloudPlan(int(r.plan.status), path[r.plan.path_offset: r.plan.path_offset + r.plan.path_len].copy(), int(r.plan.n_expanded),
                          int(r.plan.n_pushed), int(r.plan.n_discarded_closed), np.float32(r.plan.g_goal), int(r.plan.host_waits),
                          int(r.n_knn_fallbacks), int(r.n_lethal_skipped), int(r.n_los_tested), int(r.n_los_blocked), int(r.n_los_capped),
                          int(r.max_successors)) for r in res]

    def plan_on_cloud(self, start: int, goal: int) -> "CloudPlan":
        return self.plan_many_on_cloud([start], [goal])[0]

    def close(self):
        pass      # the context owns the device state
