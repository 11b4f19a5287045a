"""Regenerate tests/golden/trace_iow_*.npz: IOW-03 scenes, 2048 ray queries each, and the reference
answers of tests/trace_iow_ref.c (the CPU oracle's launch_ray per query).

Each fixture is self-contained: types (N,), records (N, 24), rays (Q, 8 float32 = rt_ray), hits
(Q, 8 uint32 = rt_hit), cut_id (Q,: for a query whose tmax was drawn around a real hit's t, the id
the same query hits with tmax = 32000; else -1) and ovf (Q, bool: the queries built to overflow
the walk's link stack -- `shells`: from the spheres' common centre; `chain`: along the row from its
small end).  Run from the repo root (needs gcc and the built librt_hip.so
for the packer and the host BVH build; no GPU):
    python tests/golden/make_trace_iow_golden.py
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "raytracing-tests_amd"), os.path.dirname(HERE)]

import rt_amd as R  # noqa: E402
import trace_iow_ref as T  # noqa: E402

Q = 2048
FAR = 32000.0
ELL, CUB = R.RT_IOW_ELLIPSOID, R.RT_IOW_CUBOID


def _pack(objs):
    """objs: (type, position, rotation_deg, scale, refractive_index) -> types, records."""
    arr = (R.RtGeomDesc * len(objs))()
    for d, (ty, pos, rot, scale, ri) in zip(arr, objs):
        d.type = ty
        for k in range(3):
            d.position[k] = d.last_position[k] = float(pos[k])
            d.rotation_deg[k], d.scale[k] = float(rot[k]), float(scale[k])
            d.color[k] = 0.5
        d.refractivity, d.reflectivity, d.refractive_index = 0.3, 0.3, float(ri)
    out = R.pack(arr, len(objs), R.RT_STAGE_IOW03)
    return out["types"], out["records"]


def scene_final():
    sc = R.make_scene(R.PRESET_IOW03_FINAL, 20250131, 0)
    return sc.types, sc.records


def scene_final2():
    ty, rec = scene_final()
    rec2 = rec.copy()
    rec2[:, 0] += np.float32(40.0)
    return np.concatenate([ty, ty]), np.concatenate([rec, rec2])


def scene_ref3():
    sc = R.make_scene(R.PRESET_IOW03_REF3, 0, 0)
    return sc.types, sc.records


def scene_one():
    return _pack([(ELL, (0.5, 0.25, -1.0), (0, 0, 0), (1.5, 1.0, 1.25), 1.3)])


def scene_rot():
    rng = np.random.default_rng(61)
    return _pack([(ELL if i % 2 == 0 else CUB, rng.uniform(-1, 1, 3) * (10.0, 3.0, 10.0), rng.uniform(-90, 90, 3),
                   rng.uniform(0.3, 2.0, 3), 1.0 + 0.01 * (i % 50)) for i in range(300)])


def scene_dups():
    rng = np.random.default_rng(62)
    base = [(ELL if i % 3 else CUB, rng.uniform(-1, 1, 3) * (7.0, 2.0, 7.0), (0, 0, 0), (rng.uniform(0.4, 1.2),) * 3,
             1.0 + 0.01 * i) for i in range(100)]
    return _pack(base + base + base)  # objects i, i + 100 and i + 200 share one record: every hit ties in t


def scene_touch():
    objs = [(CUB, (x, y, z), (0, 0, 0), (1, 1, 1), 1.0 + 0.01 * ((x + 7 * y + 49 * z) % 64))
            for z in range(6) for y in range(7) for x in range(7) if (x + y + z) % 5 != 4]  # a few holes
    return _pack(objs)


def scene_shells():
    return _pack([(ELL, (1.0, 2.0, -3.0), (0, 0, 0), (0.2 + 0.05 * i,) * 3, 1.0 + 0.001 * i) for i in range(450)])


def scene_chain():
    """A row of spheres growing by 1.3 along +x.  The culling BVH peels the largest off level by level,
    so it is a chain; a ray along the row from the small end enters the rest first at every level and
    leaves three siblings on the stack each time: more than 13 entries, and more than 29."""
    return _pack([(ELL, (3.0 * 1.3 ** i, 0, 0), (0, 0, 0), (0.8 * 1.3 ** i,) * 3, 1.0 + 0.01 * i) for i in range(64)])


SCENES = {"final": scene_final, "final2": scene_final2, "ref3": scene_ref3, "one": scene_one, "rot": scene_rot,
          "dups": scene_dups, "touch": scene_touch, "shells": scene_shells, "chain": scene_chain}
# objects and 4-wide nodes of rt_iow_host_build (0 nodes: no BVH, the linear loop)
SIZES = {"final": (486, 235), "final2": (972, 530), "ref3": (3, 1), "one": (1, 0)}
SEEDS = {name: 200 + i for i, name in enumerate(SCENES)}


def _unit(v):
    return v / np.linalg.norm(v)


def make_rays(name, types, rec, seed, n=Q):
    """Eight kinds in turn; ratio holds random bits.  Returns rays, the queries to cut, the overflow mask."""
    rng = np.random.default_rng(seed)
    pos, scale = rec[:, 0:3].astype(np.float64), rec[:, 12:15].astype(np.float64)
    small = np.flatnonzero(scale.max(1) < 50.0)  # aim at the objects, not at a ground slab
    if len(small) == 0:
        small = np.arange(len(rec))
    lo, hi = (pos - scale)[small].min(0), (pos + scale)[small].max(0)
    mid, ext = (lo + hi) / 2, np.maximum((hi - lo) / 2, 1.0)
    cubs = np.flatnonzero(types == CUB)
    rays = np.zeros(n, T.RAY_DTYPE)
    cut = np.zeros(n, bool)
    centre = np.zeros(n, bool)
    for q in range(n):
        kind, sub = q % 8, (q // 8)
        g = int(rng.choice(small))
        M = rec[g, 3:12].astype(np.float64).reshape(3, 3).T  # the shader's M * v
        tmax = FAR
        o = mid + ext * rng.uniform(1.5, 2.5) * _unit(rng.normal(size=3) + (0, 1.0, 0))  # a camera around the scene
        aim = pos[g] + 0.3 * scale[g] * rng.uniform(-1, 1, 3)
        d = _unit(aim - o)
        if kind == 0:    # camera-like, towards the scene
            d = _unit(mid + ext * rng.uniform(-1.1, 1.1, 3) - o)
        elif kind == 1:  # starts inside an object (shells: at the common centre)
            o = pos[g] + 0.2 * scale[g].min() * rng.uniform(-1, 1, 3)
            d = _unit(rng.normal(size=3))
            if name == "shells":
                o, centre[q] = pos[g], True
            elif name == "chain":
                o, d, centre[q] = np.array([0.0, *rng.uniform(-0.3, 0.3, 2)]), np.array([1.0, 0, 0]), True
                tmax = np.inf  # (32000 would cull the far half of the row before the walk starts)
        elif kind == 2:  # starts on a cuboid face (exactly so where M is the identity), any direction
            if len(cubs):
                g = int(rng.choice(cubs))
                M = rec[g, 3:12].astype(np.float64).reshape(3, 3).T
            local = 0.5 * scale[g] * rng.uniform(-1, 1, 3)
            k = int(rng.integers(3))
            local[k] = 0.5 * scale[g][k] * float(rng.choice((-1.0, 1.0)))
            o = pos[g] + M.T @ local
            d = _unit(rng.normal(size=3))
            if sub % 2:  # ... or along the face
                d[k] = 0.0
                d = _unit(d)
        elif kind == 3:  # along an axis through an object: two zero direction components
            k, sgn = int(rng.integers(3)), float(rng.choice((-1.0, 1.0)))
            o = pos[g] + 0.3 * scale[g] * rng.uniform(-1, 1, 3)
            o[k] -= sgn * (ext[k] * 2.5 + 1.0)
            d = np.zeros(3)
            d[k] = sgn
        elif kind == 4:  # not normalised: lengths 0.5 and 2, |d|^2 just inside and outside (0.998, 1.002)
            d = d * (0.5, 2.0, np.sqrt(0.9981), np.sqrt(0.9979), np.sqrt(1.0019), np.sqrt(1.0021))[sub % 6]
        elif kind == 5:  # degenerate directions (misses) and limits
            m = sub % 8
            if m == 0:
                d = np.zeros(3)
            elif m == 1:
                d[int(rng.integers(3))] = np.nan
            else:
                tmax = (np.inf, 0.0, -1.0, np.nan, np.inf, FAR)[m - 2]
        elif kind == 6:  # a limit around the hit's t (set once the uncut answer is known)
            cut[q] = True
        rays[q]["o"], rays[q]["d"] = o.astype(np.float32), d.astype(np.float32)
        rays[q]["tmax"] = np.float32(tmax)
    rays["ratio"] = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32)
    return rays, cut, centre, rng


def main():
    only = set(sys.argv[1:])
    lim = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE)
              if f.startswith("trace_") and not f.startswith("trace_iow_") and f.endswith(".npz"))
    with tempfile.TemporaryDirectory() as tmp:
        lib = T.build(tmp)
        for name in T.SCENES:
            if only and name not in only:
                continue
            types, rec = SCENES[name]()
            nodes = R.iow_host_build(types, rec, len(types))["wide_nodes"]
            if name in SIZES:
                assert (len(types), nodes) == SIZES[name], (name, len(types), nodes)
            if name in ("shells", "chain"):
                assert 0 < nodes <= 240, nodes  # the LDS path
            rays, cut, centre, rng = make_rays(name, types, rec, SEEDS[name])
            uncut = T.run(lib, types, rec, rays)
            cut_id = np.full(Q, -1, np.int32)
            for q in np.flatnonzero(cut & (uncut["id"] >= 0)):
                cut_id[q] = uncut["id"][q]
                rays[q]["tmax"] = np.float32(uncut["t"][q] * rng.uniform(0.5, 1.5))
            hits = T.run(lib, types, rec, rays)
            rate = float((hits["id"] >= 0).mean())
            assert 0.10 <= rate <= 0.90, (name, rate)
            kept = cut_id >= 0
            assert (hits["id"][kept & (hits["id"] >= 0)] == cut_id[kept & (hits["id"] >= 0)]).all()
            assert (hits["id"][kept] < 0).any() and (hits["id"][kept] >= 0).any(), name
            out = {"types": types, "records": rec, "rays": rays.view(np.float32).reshape(-1, 8),
                   "hits": hits.view(np.uint32).reshape(-1, 8), "cut_id": cut_id, "ovf": centre}
            path = os.path.join(HERE, f"trace_iow_{name}.npz")
            np.savez_compressed(path, **out)
            assert os.path.getsize(path) <= lim, (name, os.path.getsize(path))
            print(name, "n", len(types), "nodes", nodes, "hit fraction", round(rate, 3),
                  "ids hit", len(np.unique(hits["id"])) - 1, "cut", int(kept.sum()),
                  "cut misses", int((hits["id"][kept] < 0).sum()), "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
