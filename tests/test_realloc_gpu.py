"""The context's buffers that are allocated again during its life (dev_realloc, csrc/dev_memory.hip.h): the rollout's state
arrays, which grow when a tick's horizon needs more (trajectory, step) pairs than they hold, and the exchange buffers,
which come back with every comm_init / comm_loopback after a comm_destroy.  In both cases the context must afterwards
deliver, bit for bit, what a fresh context delivers that only ever saw the later state."""
import numpy as np
import pytest

from dddmr_navigation_amd import configs, scenes
from dddmr_navigation_amd.local_planner import LocalPlanner

pytestmark = pytest.mark.gpu


def _fields(r):
    return (r.planner_state, r.best_index, r.best_cost, r.vx, r.vy, r.wz, r.key, r.n_samples, r.n_local, r.n_points_binned)


def _command(r):
    return (r.planner_state, r.best_index, r.best_cost, r.vx, r.vy, r.wz)


def test_state_arrays_grow_for_a_longer_horizon():
    """55 trajectories (the playground's window: v <= 0.5, |w| <= 0.3, so a horizon of 12 * sim_time + 1 steps).  At
    sim_time 1 the first tick needs 55 * 13 = 715 pairs and the arrays are made for 715 + 715 / 4 + 1024 = 1917; at
    sim_time 5 the second needs 55 * 61 = 3355, so they are freed and made again between the two ticks."""
    pg = scenes.playground_scene()
    short = configs.dd_simple_shipped(sim_time=1.0, name="short")
    long_ = configs.dd_simple_shipped(sim_time=5.0, name="long")
    cloud = np.concatenate([pg.cloud, scenes.bench_scene("C1").cloud[:300]])

    def ticks(names):
        out = []
        with LocalPlanner([short, long_], max_points=len(cloud)) as lp:
            lp.set_cloud(cloud)
            lp.setPlan(pg.plan)
            for name in names:
                res = lp.tick(name, pg.tick)
                out.append((_fields(res),) + tuple(a.copy() for a in lp.debug()))
        return out

    first, second = ticks(["short", "long"])
    (fresh,) = ticks(["long"])
    n = len(first[2])
    assert n == len(second[2]) == 55 and 0 < first[2].max() <= 13
    assert n * int(second[2].max()) > 715 + 715 // 4 + 1024, "the second tick fits the first tick's arrays: nothing grew"
    assert second[0] == fresh[0]
    np.testing.assert_array_equal(second[1].view(np.int64), fresh[1].view(np.int64))
    np.testing.assert_array_equal(second[2], fresh[2])
    np.testing.assert_array_equal(second[3].view(np.int32), fresh[3].view(np.int32))


def test_exchange_buffers_come_back_after_comm_destroy():
    """One rank of 2 in loopback mode with the peer's winner words set, then comm_destroy, then loopback again: the new slot
    vectors start without the peer's words (the tick returns this shard's own winner) and, once the words are set again,
    the tick returns what a context returns that entered loopback once."""
    sc = scenes.bench_scene("C1")
    name = sc.theory.name.decode()
    cloud = sc.cloud

    def rank(r):
        lp = LocalPlanner([sc.theory], max_points=len(cloud), rank=r, world_size=2)
        lp.set_cloud(cloud)
        lp.setPlan(sc.plan)
        return lp

    # the rank under test is the one whose own winner loses (or that has none), so the peer's words decide the result
    words = []
    for r in range(2):
        with rank(r) as lp:
            words.append(lp.winner_words(lp.tick(name, sc.tick)))
    me = 0 if words[0] > words[1] else 1
    peer, peer_words = 1 - me, words[1 - me]
    assert peer_words[0] != 2**63 - 1, "the scene has a winner"
    with rank(me) as once:
        own = _command(once.tick(name, sc.tick))
        once.comm_loopback()
        once.comm_loopback_set_peer(peer, peer_words)
        want = _fields(once.tick(name, sc.tick))
        want_costs = once.debug()[0].copy()
    assert want[1] >= 0 and want[1] != own[1]
    with rank(me) as lp:
        lp.comm_loopback()
        lp.comm_loopback_set_peer(peer, peer_words)
        assert _fields(lp.tick(name, sc.tick)) == want
        lp.comm_destroy()
        assert _command(lp.tick(name, sc.tick)) == own
        lp.comm_loopback()
        assert lp.comm_ranks() == 2
        assert _command(lp.tick(name, sc.tick)) == own         # fresh slots: nobody's words but this rank's
        lp.comm_loopback_set_peer(peer, peer_words)
        assert _fields(lp.tick(name, sc.tick)) == want
        np.testing.assert_array_equal(lp.debug()[0].view(np.int64), want_costs.view(np.int64))
