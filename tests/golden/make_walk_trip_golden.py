"""Regenerate tests/golden/trace_walk_*.npz: ray-query fixtures (the trace_*.npz format of
make_trace_golden.py, at most 2048 queries each) aimed at the state transitions of the wide walk's
trip (csrc/rt_inw_walk.hpp: inw_traverse_wide) inside one 64-query wave:

  walk_chain   a row of growing spheres whose culling tree is a chain: rays along the row overflow
               the walk's node stack (cap 37 in the query kernel) beside rays that do not;
  walk_pile    concentric and scattered spheres: rays through the pile hold a pending leaf again and
               again while lanes with one or no leaf have long finished;
  walk_moving  moving spheres with two time-bin trees: ratios 0, just below 0.5, 0.5 and 1; lanes
               the walk refuses (a zero direction component, a non-finite reciprocal, a per-ray term
               -o/d that overflows with the fused cull) beside lanes it takes;
  walk_face    duplicated unrotated spheres (a scene with sphere records) hit where the surface
               touches the leaf box: t <= the box entry with a tie behind it, the leaf-entry
               guard's case, in every wave;
  walk_three, walk_one   the stack empties on the first pop; the root is a leaf.

Every property is asserted here, on the CPU, with a model of the walk's stack (walk_model) over the
host-built 4-wide nodes (rt_debug_time_bins) where it needs one.  Run from the repo root (needs gcc
and the built librt_hip.so; no GPU):
    python tests/golden/make_walk_trip_golden.py
"""
import ctypes as C
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "raytracing-tests_amd"), os.path.dirname(HERE)]

import rt_amd as R  # noqa: E402
import trace_ref as T  # noqa: E402
import walk_trip_cases as W  # noqa: E402
from make_trace_golden import _pack, _spheres, _unit  # noqa: E402

FAR = 32000.0
ELL = R.RT_INW_ELLIPSOID
Z = np.zeros(3)


def scene_chain():
    """The culling tree peels the largest spheres off level by level (three leaves and the rest per
    node); the reference's LBVH over the same row stays within the 40-float stack (dfs_high 40), so
    the walk's own condition holds.  Growth, spacing and count were searched for that pair."""
    return _pack([(ELL, (3.6 * W.CHAIN_GROWTH ** i, 0, 0), (3.6 * W.CHAIN_GROWTH ** i, 0, 0), Z,
                   (0.68 * W.CHAIN_GROWTH ** i,) * 3) for i in range(W.CHAIN_N)]), 1


def scene_pile():
    objs = [(ELL, Z, Z, Z, (0.3 + 0.1 * i,) * 3) for i in range(24)]
    objs += _spheres(np.random.default_rng(61), 12, half=(6.0, 2.0, 6.0), r=(0.3, 0.8), move=0.0)
    return _pack(objs), 1


def scene_moving():
    return _pack(_spheres(np.random.default_rng(71), 600, half=(14.0, 3.0, 14.0), r=(0.3, 1.0), move=1.5)), 1


def scene_face():
    """Unrotated spheres only, so the scene has sphere records (rt_debug_sphere_records accepts it)
    and inw_sphere_records switches between the sphere-record leaf test and the full-record one."""
    rng = np.random.default_rng(81)
    objs = []
    for i in range(60):
        p = np.round(rng.uniform(-1, 1, 3) * (8.0, 2.0, 8.0) * 4) / 4  # quarter units: exact box planes
        s = float(rng.integers(2, 7)) / 4
        objs.append((ELL, p, p, Z, (s, s, s)))
    return _pack(objs + objs), 1  # object i and i + 60 coincide: every hit has a tie behind it


def scene_small(n, seed):
    return _pack(_spheres(np.random.default_rng(seed), n, half=(2.0, 1.0, 2.0), r=(0.5, 1.2), move=0.2)), 1


def _ray(o, d, tmax=FAR, ratio=0.0):
    r = np.zeros((), T.RAY_DTYPE)
    r["o"], r["d"], r["tmax"], r["ratio"] = np.asarray(o, np.float32), np.asarray(d, np.float32), tmax, ratio
    return r


def _aimed(rng, geom, aabbs, ratio=0.0, spread=0.3):
    lo, hi = aabbs[:, :3].min(0).astype(np.float64), aabbs[:, 3:].max(0).astype(np.float64)
    mid, ext = (lo + hi) / 2, np.maximum((hi - lo) / 2, 1.0)
    f = geom[int(rng.integers(len(geom)))].astype(np.float64)
    centre = f[0:3] - f[15:18] * (1.0 - ratio)
    o = mid + ext * 1.5 * _unit(rng.normal(size=3))
    return _ray(o, _unit(centre + spread * f[12:15] * rng.uniform(-1, 1, 3) - o), FAR, ratio)


def rays_chain(geom, aabbs, n=512):
    """Per wave of 64: lanes 0-15 along the row from its small end (they overflow), the rest aimed at
    single spheres from the side (a few node steps)."""
    rng = np.random.default_rng(301)
    out = []
    for q in range(n):
        if q % 64 < 16:
            out.append(_ray((0.0, *rng.uniform(-0.2, 0.2, 2)), _unit((1.0, *rng.uniform(-2e-4, 2e-4, 2))), np.inf))
        else:
            f = geom[int(rng.integers(len(geom)))].astype(np.float64)
            o = f[0:3] + (0.0, 4.0 * f[12], 0.5 * f[12])
            out.append(_ray(o, _unit(f[0:3] + 0.3 * f[12] * rng.uniform(-1, 1, 3) - o)))
    return np.array(out)


def rays_pile(geom, aabbs, n=512):
    """Per wave: even lanes through the pile's centre (two dozen leaves each), odd lanes aimed at a
    scattered sphere or past everything."""
    rng = np.random.default_rng(302)
    out = []
    for q in range(n):
        o = 12.0 * _unit(rng.normal(size=3))
        if q % 2 == 0:
            out.append(_ray(o, _unit(0.05 * rng.uniform(-1, 1, 3) - o)))
        elif q % 4 == 1:
            f = geom[24 + int(rng.integers(12))].astype(np.float64)
            out.append(_ray(o, _unit(f[0:3] - o)))
        else:
            out.append(_ray(o, _unit(o + rng.normal(size=3) * 0.2)))  # outward: nothing ahead
    return np.array(out)


def rays_moving(geom, aabbs, n=1024):
    """Ratios 0, below 0.5, 0.5, 1 in turn; of every 8 lanes one refused by the walk, in three ways."""
    rng = np.random.default_rng(303)
    out = []
    for q in range(n):
        r = _aimed(rng, geom, aabbs, float(W.RATIOS[q % 4]))
        kind = (q // 4) % 8
        if kind == 3:    # a zero direction component
            r["d"][int(rng.integers(3))] = 0.0
        elif kind == 5:  # a subnormal one: its reciprocal is infinite
            r["d"][int(rng.integers(3))] = np.float32(1e-40)
        elif kind == 7:  # finite reciprocal (~1e38), but -o/d overflows: the fused cull's refusal
            k = int(rng.integers(3))
            r["d"][k] = np.float32(2e-38)
            r["o"][k] = np.float32(20.0)
        out.append(r)
    return np.array(out)


def rays_face(geom, aabbs, n=1024):
    """Three lanes of four aimed at the point where a sphere touches its leaf box, from outside,
    with every direction component nonzero; the fourth into a sphere."""
    rng = np.random.default_rng(304)
    out = []
    for q in range(n):
        g = int(rng.integers(len(geom) // 2))
        f = geom[g].astype(np.float64)
        k, sgn = int(rng.integers(3)), float(rng.choice((-1.0, 1.0)))
        touch = f[0:3].copy()
        touch[k] += sgn * f[12 + k]
        if q % 4 == 3:  # every fourth lane: an ordinary hit, aimed into the sphere
            touch = f[0:3] + 0.5 * f[12:15] * rng.uniform(-1, 1, 3)
        off = rng.uniform(-0.5, 0.5, 3)
        off[k] = sgn * rng.uniform(2.0, 6.0)
        o = np.round((touch + off) * 8) / 8
        o[(touch - o).astype(np.float32) == 0] += 0.125
        out.append(_ray(o, (touch - o).astype(np.float32)))  # not normalised: t = 1 at the touch point
    return np.array(out)


def rays_small(geom, aabbs, n=256):
    rng = np.random.default_rng(305 + len(geom))
    return np.array([_aimed(rng, geom, aabbs, (q % 5) / 4.0, spread=1.5) for q in range(n)])


SCENES = {"walk_chain": (scene_chain, rays_chain), "walk_pile": (scene_pile, rays_pile),
          "walk_moving": (scene_moving, rays_moving), "walk_face": (scene_face, rays_face),
          "walk_three": (lambda: scene_small(3, 33), rays_small), "walk_one": (lambda: scene_small(1, 31), rays_small)}


def main():
    only = set(sys.argv[1:])
    with tempfile.TemporaryDirectory() as tmp:
        lib = T.build(tmp)
        for name in W.FIXTURES:
            if only and name not in only:
                continue
            (geom, aabbs, nodes), layout = SCENES[name][0]()
            rays = SCENES[name][1](geom, aabbs)
            assert len(rays) <= 2048
            out = {"geom": geom, "aabbs": aabbs, "nodes": nodes, "layout": np.int32(layout),
                   "rays": rays.view(np.float32).reshape(-1, 8)}
            for inv in (0, 1):
                hits, ctr = T.run(lib, geom, nodes, layout, rays, inv)
                out[f"hits{inv}"] = hits.view(np.uint32).reshape(-1, 8)
                out[f"ctr{inv}"] = ctr
            path = os.path.join(HERE, f"trace_{name}.npz")
            np.savez_compressed(path, **out)
            print(name, "n", len(geom), "queries", len(rays), W.check(name, T.load_fixture(name)), "bytes",
                  os.path.getsize(path))


if __name__ == "__main__":
    main()
