"""Scenes and queries for the wide walk's leaf takes (csrc/rt_inw_walk.hpp: inw_traverse_wide takes
a node step's nearest-child leaf in the step's own trip), and a CPU model of one lane that says which
state transitions a query goes through.  tests/test_walk_takes_ref.py asserts on the CPU that the
cases are there; tests/test_gpu_walk_takes.py runs them on the GPU."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.join(HERE, "golden") not in sys.path:
    sys.path.append(os.path.join(HERE, "golden"))

import rt_amd as R  # noqa: E402
import trace_ref as T  # noqa: E402
import walk_trip_cases as W  # noqa: E402
from make_trace_golden import _pack, _spheres, _unit  # noqa: E402

F = np.float32
DONE = -(2 ** 31)
SIZES = (1, 2, 3, 5, 17)
SEEDS = {1: 31, 2: 32, 3: 33, 5: 35, 17: 47}
N_RAYS = 256  # four waves


class Scene:
    """A packed scene (what R.trace takes) with its queries."""

    def __init__(self, geom, aabbs, nodes, rays, layout=1):
        self.geom, self.aabbs, self.nodes, self.layout = geom, aabbs, nodes, layout
        self.n = geom.shape[0]
        self.rays = rays

    def as_dict(self):
        return {"geom": self.geom, "nodes": self.nodes, "aabbs": self.aabbs, "layout": self.layout}


def _ray(o, d, tmax=32000.0, ratio=0.0):
    r = np.zeros((), T.RAY_DTYPE)
    r["o"], r["d"], r["tmax"], r["ratio"] = np.asarray(o, F), np.asarray(d, F), tmax, ratio
    return r


def small_scene(n):
    """n slowly moving spheres in a slab, close enough that rays cross several boxes.  Per wave of
    64: three lanes of four aimed at an object from outside the slab (at other angles, so the
    nearest child of the root differs between lanes), every fourth lane starting inside the slab."""
    rng = np.random.default_rng(SEEDS[n])
    geom, aabbs, nodes = _pack(_spheres(rng, n, half=(3.0, 1.0, 3.0), r=(0.5, 1.2), move=0.2))
    lo, hi = aabbs[:, :3].min(0).astype(np.float64), aabbs[:, 3:].max(0).astype(np.float64)
    mid, ext = (lo + hi) / 2, np.maximum((hi - lo) / 2, 1.0)
    rays = []
    for q in range(N_RAYS):
        ratio = (q % 5) / 4.0
        f = geom[int(rng.integers(n))].astype(np.float64)
        centre = f[0:3] - f[15:18] * (1.0 - ratio)
        if q % 4 == 3:
            o = mid + ext * rng.uniform(-0.9, 0.9, 3)
        else:
            o = mid + ext * 1.6 * _unit(rng.normal(size=3))
        rays.append(_ray(o, _unit(centre + 1.5 * f[12:15] * rng.uniform(-1, 1, 3) - o), 32000.0, ratio))
    return Scene(geom, aabbs, nodes, np.array(rays))


def chain_scene():
    """walk_chain's row of growing spheres (its culling tree is a chain) with queries along the row
    from its small end, started at every sphere of the row's first half: they reach the walk
    stack's cap (37 entries in the query kernel) with different numbers of entries to spare, so
    some overflow in a trip that takes a leaf and some in a trip that does not.  Three lanes of
    four; the fourth is aimed at one sphere from the side and stays far from the cap."""
    d = T.load_fixture("walk_chain")
    geom = d["geom"]
    rng = np.random.default_rng(401)
    rays = []
    for q in range(N_RAYS):
        if q % 4 == 3:
            f = geom[int(rng.integers(len(geom)))].astype(np.float64)
            o = f[0:3] + (0.0, 4.0 * f[12], 0.5 * f[12])
            rays.append(_ray(o, _unit(f[0:3] + 0.3 * f[12] * rng.uniform(-1, 1, 3) - o)))
        else:
            x0 = 0.0 if q % 8 < 4 else 3.6 * W.CHAIN_GROWTH ** (q % 24) * 0.5
            rays.append(_ray((x0, *rng.uniform(-0.2, 0.2, 2)), _unit((1.0, *rng.uniform(-2e-4, 2e-4, 2))), np.inf))
    return Scene(geom, d["aabbs"], d["nodes"], np.array(rays), d["layout"])


def lane_events(wn, links, root, o, d, tmax, cap=W.WALK_CAP):
    """One lane of inw_traverse_wide (unfused cull), trip by trip, up to the trip after which it
    waits on a second leaf, ends or overflows.  Until then no leaf has been tested, so the culling
    limit is the initial one and what the lane does cannot depend on the other lanes of its wave.
    Returns (events, trips): the names of the transitions it went through, and
    for each trip 'step', 'take' (a node step whose nearest child is a leaf it can take) or 'idle'."""
    o, d = o.astype(F), d.astype(F)
    ev, trips = set(), []
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        inv = F(1.0) / d
        lim = F(F(tmax) * F(1.0001) + F(1e-3))
        stack, cur, pend = [], int(root), -1
        while True:
            stepped = cur > 0
            nxt, miss = cur, False
            if stepped:
                nd = wn[cur - 1]
                t = []
                for c in range(4):
                    te, tx = F(-np.inf), F(np.inf)
                    for a in range(3):
                        s = 1 if d[a] < 0 else 0
                        near, far = nd[4 * (a + 3 * s) + c], nd[4 * (a + 3 * (1 - s)) + c]
                        te, tx = max(te, F((near - o[a]) * inv[a])), min(tx, F((far - o[a]) * inv[a]))
                    t.append(te if max(te, F(-1e-3)) <= min(tx, lim) else W.MISS)
                k = [int(v) for v in links[cur - 1]]
                for a, b in ((0, 1), (2, 3), (0, 2), (1, 3), (1, 2)):
                    W._cswap(t, k, a, b)
                pushed = [k[j] for j in (3, 2, 1) if t[j] != W.MISS]
                stack += pushed
                nxt, miss = k[0], t[0] == W.MISS
                if not miss:
                    if nxt <= 0 and any(v > 0 for v in pushed):
                        ev.add("near_leaf_far_node")
                    if nxt > 0 and any(v <= 0 for v in pushed):
                        ev.add("near_node_far_leaf")
            take = nxt <= 0 and nxt != DONE and not miss and pend < 0
            trips.append("take" if take and stepped else "step" if stepped else "idle")
            if take and stepped:
                ev.add("step_take")
            if take:
                pend = -nxt
            if len(stack) > cap:
                ev.add("overflow_taking" if take and stepped else "overflow_other")
                return ev, trips
            if take or miss:
                if not stack:
                    ev.add("empty_in_taking_trip" if take else "empty_after_miss")
                    return ev, trips
                cur = stack.pop()
                if cur <= 0:
                    if stack and stack[-1] <= 0:
                        ev.add("leaf_under_leaf")
                    if pend >= 0:
                        ev.add("popped_leaf_waits")
                        return ev, trips
                    ev.add("popped_leaf_free")
                    ev.add("popped_leaf_last" if not stack else
                           "free_leaf_over_leaf" if stack[-1] <= 0 else "free_leaf_over_node")
            else:
                cur = nxt
                if cur <= 0:
                    ev.add("near_leaf_waits")
                    return ev, trips


def events_of(sc):
    """lane_events of every query over the scene's one tree (inw_time_bins = 0), and the root's links."""
    wn, links, _ = W.wide_nodes(sc.as_dict(), bins=1)
    info = R.inw_host_build(sc.nodes, sc.n)
    if sc.n == 1:
        return None, None, info
    out = [lane_events(wn, links, 1, sc.rays["o"][q], sc.rays["d"][q], sc.rays["tmax"][q]) for q in range(len(sc.rays))]
    return out, links, info
