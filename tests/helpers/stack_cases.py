"""The update sequence tests/test_stack_cpu.py and tests/test_stack_gpu.py share: a lidar on source 0 fed a fresh scan at a
moving pose each update, two depth cameras on sources 1 and 2 (the rig and boxes of depth_layer_cases), a static host
layer.  Everything expected comes from the restatements alone: oracle.feed + oracle.MarkingOracle for the lidar layer,
depth_layer_ref (through depth_layer_cases.built) for the depth layer, stack_ref for the stack.  CPU only."""
import numpy as np

from dddmr_navigation_amd import _capi as K, marking, scenes
import oracle

import depth_layer_cases as cases
import depth_mark_cases as mc
import stack_ref as S

A, B, C = cases.A, cases.B, cases.C
Up = cases.Up
# The robot drives ahead and turns a little.  The cameras see depth_layer_cases' sparse scene (a box that always stands
# and boxes that come and go), the lidar two pillars that stand still in the global frame: one beside the first box, so
# that both layers are lethal there at once, one behind the robot where only the lidar sees anything.  Small scenes keep
# the changed set of an update well below a tenth of the ground's 4225 nodes once the first update has filled the stack.
SEQUENCE = cases.Case("stack_sequence", 552, [Up(yaw=0.05, boxes=A), Up(yaw=0.10, dx=0.2, boxes=B), Up(yaw=0.15, dx=0.4, boxes=()),
                                              Up(yaw=0.10, dx=0.6, boxes=C), Up(yaw=0.05, dx=0.8, boxes=A)], cams=2, lidar=True, sparse=True,
                      min_size=5)
cases.BY_NAME[SEQUENCE.name] = SEQUENCE
PILLARS = ((2.0, 0.75), (-2.0, -1.5))


def lidar_scene():
    rng = np.random.Generator(np.random.PCG64(77))
    out = []
    for cx, cy in PILLARS:
        a = rng.uniform(0.0, 2.0 * np.pi, 4000)
        out.append(np.stack([cx + 0.1 * np.cos(a), cy + 0.1 * np.sin(a), rng.uniform(0.0, 1.4, 4000)], axis=1))
    return (np.concatenate(out, axis=0) + SEQUENCE.shift).astype(np.float32)


def lidar_feed(k, t_gb):
    """a fresh scan of the pillars from the pose of update k, in the sensor's frame (the base's axes)"""
    x, y, z = t_gb[:3]
    scan = scenes.lidar_scan(lidar_scene(), sensor_xyz=(x + mc.TBS_LIDAR[0], y + mc.TBS_LIDAR[1], z + mc.TBS_LIDAR[2]), seed=5 + k)
    yaw = 2.0 * np.arctan2(t_gb[5], t_gb[6])
    c, s_ = np.cos(yaw), np.sin(yaw)
    rot = np.array([[c, s_, 0.0], [-s_, c, 0.0], [0.0, 0.0, 1.0]])          # global axes -> base axes
    return dict(sid=0, kind="lidar", data=(scan.astype(np.float64) @ rot.T).astype(np.float32), t_bs=mc.TBS_LIDAR, t_gb=t_gb)


RESET_AT = 3                                   # test_stack_gpu's reset test resets before this update
WINDOW, HEIGHT = 5.0, 2.0                      # the lidar feed's
ORDER = (K.STACK_HOST0, K.STACK_LIDAR, K.STACK_DEPTH)       # plugin order: static layer first, as the shipped configuration lists it
POS = {layer: p for p, layer in enumerate(ORDER)}


def marking_config():
    return marking.shipped_config(max_markings=1 << 12, max_cluster_points=1 << 16, inflation_radius=1.0)


def static_layer(ground):
    """A static layer's dGraph as the host would compute it: the distance to a wall 2.5 m left of the first pose, within the
    inflation radius; elsewhere the layer's maximum.  Three nodes carry values only a host layer can have."""
    g = ground.astype(np.float64)
    d = np.abs(g[:, 1] - (g[:, 1].mean() + 2.5))
    v = np.where(d < 1.5, d, 9999.0)
    v = np.concatenate([v, [9999.0]])
    v[5], v[6], v[7] = np.nan, np.inf, 123456.0
    return v


_BUILT = {}


def built(reset_at=None):
    """-> dict: case, ups (every update with a lidar feed first), ground, static, and per update k: lidar_obs, depth result
    (depth_layer_cases), lidar stats / voxels / dgraph / lethal, stacked (values, mask), changed, lethal_nodes"""
    if reset_at in _BUILT:
        return _BUILT[reset_at]
    case, ups0, ground, depth_res = cases.built(SEQUENCE.name)
    ups = []
    for k, u in enumerate(ups0):
        ups.append(dict(u, feeds=[lidar_feed(k, u["t_gb"])] + [f for f in u["feeds"] if f["kind"] != "lidar"]))
    no_map = np.zeros((0, 3), np.float32)
    mo = oracle.MarkingOracle(marking_config(), ground, no_map)
    whole = oracle.MarkingOracle(marking_config(), ground, no_map)     # fed the whole aggregate, as marking_update would be
    dref = cases.layer_ref(case, ground) if reset_at is not None else None
    static = static_layer(ground)
    n = len(ground)
    layers = [None] * 3
    layers[POS[K.STACK_HOST0]] = (static, None)
    layers[POS[K.STACK_LIDAR]] = (mo.dgraph(), mo.lethal())
    fresh_depth = (np.full(n + 1, 9999.0), np.zeros(n + 1, bool))
    layers[POS[K.STACK_DEPTH]] = fresh_depth
    # what stack_create publishes: the layers as created, the host slot still unset
    before = S.stacked([(None, None) if p == POS[K.STACK_HOST0] else l for p, l in enumerate(layers)])
    out = []
    for k, u in enumerate(ups):
        lidar_obs = oracle.feed(u["feeds"][0]["data"], mc.TBS_LIDAR, u["t_gb"], WINDOW, HEIGHT)[:, :3]
        if reset_at == k:
            mo.reset()
            dref.reset()
            layers[POS[K.STACK_LIDAR]] = (mo.dgraph(), mo.lethal())
            layers[POS[K.STACK_DEPTH]] = fresh_depth
            before = S.stacked(layers)      # what stack_reset publishes; the host slot keeps its values
        st = mo.update(lidar_obs, mc.TBS_LIDAR, u["t_gb"])
        if dref is not None:
            d = depth_res[k]
            dref.update(d["frustums"], d["obs"], u["t_gb"])
            ddg, dle = dref.dgraph.copy(), dref.lethal.copy()
        else:
            ddg, dle = depth_res[k]["dgraph"], depth_res[k]["lethal"]
        whole.update(np.concatenate([lidar_obs, depth_res[k]["obs"][:, :3]], axis=0), mc.TBS_LIDAR, u["t_gb"])
        layers[POS[K.STACK_LIDAR]] = (mo.dgraph(), mo.lethal())
        layers[POS[K.STACK_DEPTH]] = (ddg, dle)
        after = S.stacked(layers)
        out.append(dict(lidar_obs=lidar_obs, lidar_stats=st, lidar_voxels=set(map(tuple, mo.voxels().tolist())),
                        lidar_dgraph=mo.dgraph(), lidar_lethal=mo.lethal(), depth_dgraph=ddg, depth_lethal=dle,
                        stacked=after, changed=S.changed(before, after),
                        lethal_nodes=S.lethal_nodes(after[1], [POS[K.STACK_LIDAR], POS[K.STACK_DEPTH]], n),
                        whole_voxels=set(map(tuple, whole.voxels().tolist()))))
        before = after
    _BUILT[reset_at] = dict(case=case, ups=ups, ground=ground, static=static, depth=depth_res, updates=out)
    return _BUILT[reset_at]
