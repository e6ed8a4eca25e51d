"""NumPy restatement of the perception stack's own arithmetic (dddmr_rollout_stack_*): the stacked minimum dGraph of
StackedPerception::get_min_dGraphValue (stacked_perception.cpp:114-126), the lethal masks and aggregateLethal (:142-155),
and the set of nodes that changed between two passes.  The layers' own arrays come from their restatements
(oracle.MarkingOracle, depth_layer_ref.LayerRef).  CPU only."""
import numpy as np

START = 99999.9          # double tmp = 99999.9 (:116)


def stacked(layers, n=None):
    """layers: the stack in plugin order, one (values, lethal) per layer; values = n float64 or None (an unset host slot),
    lethal = n bool or None (a host layer).  -> (min dGraph [n] float64, mask [n] uint8, bit p = the layer at position p)

    The minimum is the reference's loop, literally: v = 99999.9; for each layer: v = (x < v) ? x : v, which is
    std::min(tmp, x).  A NaN never compares less, so it leaves v alone; nothing comes out above the start value."""
    if n is None:                                   # (needed only when every slot is unset)
        n = next(len(a) for pair in layers for a in pair if a is not None)
    v = np.full(n, START, np.float64)
    mask = np.zeros(n, np.uint8)
    for p, (values, lethal) in enumerate(layers):
        if values is not None:
            x = np.asarray(values, np.float64)
            with np.errstate(invalid="ignore"):
                take = x < v
            v = np.where(take, x, v)
        if lethal is not None:
            mask |= (np.asarray(lethal).astype(bool).astype(np.uint8) << np.uint8(p))
    return v, mask


def scalar_min(xs):
    """the same minimum for one node, one comparison at a time (what the vector form is checked against)"""
    v = START
    for x in xs:
        if x is not None and x < v:
            v = x
    return v


def changed(before, after):
    """(values, mask) before and after a pass -> the sorted nodes whose value BIT PATTERN or mask differs"""
    (v0, m0), (v1, m1) = before, after
    return np.flatnonzero((v0.view(np.uint64) != v1.view(np.uint64)) | (m0 != m1)).astype(np.uint32)


def lethal_nodes(mask, device_positions, n_ground):
    """aggregateLethal as node indices: for each device layer's position in plugin order, its lethal ground nodes
    (< n_ground) ascending, one list after the other"""
    out = [np.flatnonzero((mask[:n_ground] >> np.uint8(p)) & 1) for p in device_positions]
    return np.concatenate(out).astype(np.uint32) if out else np.zeros(0, np.uint32)


def apply_changes(mirror_v, mirror_m, nodes, values, masks):
    """what a consumer does with a change list"""
    mirror_v[nodes] = values
    mirror_m[nodes] = masks


class Tracker:
    """the published stacked arrays across passes: publish() is stack_create / stack_reset (no change list), step() an update"""

    def __init__(self, n_nodes):
        self.n_nodes = n_nodes
        self.values = self.mask = None

    def publish(self, layers):
        self.values, self.mask = stacked(layers, self.n_nodes)

    def step(self, layers):
        """-> the sorted changed nodes of this pass"""
        after = stacked(layers, self.n_nodes)
        ch = changed((self.values, self.mask), after)
        self.values, self.mask = after
        return ch
