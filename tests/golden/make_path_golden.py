"""Regenerate tests/golden/paths_*.npz: scenes, path queries and the reference answers of
tests/path_ref.c (the CPU oracle's sample loop restarted from each query's ray) for both child orders.

Each fixture is self-contained: geom (N, 28), aabbs (N, 6), nodes (2N - 1, 8), layout, lights (L, 7),
n_tex and tex0.. (H, W, 3|4 uint8), spp, max_bounces, rays (Q, 8 uint32 = rt_path_ray), out0 / out1
(Q, 8 uint32 = rt_path_out, invert 0 / 1), ctr0 / ctr1 (the six rt_stats counters of the reference) and,
for the cam_* fixtures, camera (pos, dir, fov_y_rad, aperture, focus_dist).  Run from the repo root
(needs gcc and the built librt_hip.so for the packers, presets and the host LBVH; no GPU):
    python tests/golden/make_path_golden.py
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "raytracing-tests_amd"), os.path.dirname(HERE), HERE]

import rt_amd as R  # noqa: E402
import path_ref as P  # noqa: E402
from make_trace_golden import make_rays  # noqa: E402  (the eight ray kinds of the trace fixtures)
from types import SimpleNamespace  # noqa: E402

Q = 2048
# (refractivity, reflectivity, refractive index, scatter refract, scatter reflect); never two strongly
# branching weights on one object: both near 0.9 make the ray tree explode
GLASS = (0.9, 0.05, 1.5, 0.0, 0.0)
MIRROR = (0.0, 0.9, 1.0, 0.0, 0.2)
DIFFUSE = (0.0, 0.0, 1.0, 0.0, 0.0)
FROSTED = (0.7, 0.2, 1.3, 0.1, 0.1)
MATS = (GLASS, MIRROR, DIFFUSE, FROSTED)


def _pack(objs):
    """objs: (type, position, last_position, rotation_deg, scale, material, colour) -> layout-1 scene."""
    arr = (R.RtGeomDesc * len(objs))()
    for d, (ty, pos, last, rot, scale, mat, col) in zip(arr, objs):
        d.type = ty
        for k in range(3):
            d.position[k], d.last_position[k] = float(pos[k]), float(last[k])
            d.rotation_deg[k], d.scale[k] = float(rot[k]), float(scale[k])
            d.color[k] = float(col[k])
        d.refractivity, d.reflectivity, d.refractive_index, d.scat_refract, d.scat_reflect = mat
    out = R.pack(arr, len(objs), R.RT_STAGE_INW01)
    return SimpleNamespace(geom=out["geom"], aabbs=out["aabbs"], nodes=out["nodes"], layout=1,
                           lights=np.zeros((0, 7), np.float32), n_lights=0, textures=None, spp=P.SPP, max_bounces=50)


def scene_glass600(shift=False):
    rng = np.random.default_rng(611)
    objs = []
    for i in range(600):
        p = rng.uniform(-1, 1, 3) * (14.0, 3.0, 14.0)
        s = rng.uniform(0.3, 1.2)
        objs.append((R.RT_INW_ELLIPSOID, p, p - rng.uniform(-0.4, 0.4, 3), (0, 0, 0), (s, s, s), MATS[i % 4],
                     rng.uniform(0.2, 1.0, 3)))
    if shift:  # the same objects one frame later: every position (and last position) moved
        rng = np.random.default_rng(612)
        objs = [(ty, p + dp, l + dp, rot, s, m, c) for (ty, p, l, rot, s, m, c) in objs
                for dp in [rng.uniform(-1.0, 1.0, 3)]]
    return _pack(objs)


def scene_pile100():
    rng = np.random.default_rng(651)
    z = np.zeros(3)
    objs = [(R.RT_INW_ELLIPSOID, z, z, z, (0.2 + 0.05 * i,) * 3, GLASS, (0.9, 0.95, 1.0)) for i in range(60)]
    for i in range(40):
        p = rng.uniform(-1, 1, 3) * (6.0, 2.0, 6.0)
        s = rng.uniform(0.3, 0.8)
        objs.append((R.RT_INW_ELLIPSOID, p, p, z, (s, s, s), MATS[i % 4], rng.uniform(0.2, 1.0, 3)))
    return _pack(objs)


def scene_mixed300():
    rng = np.random.default_rng(621)
    objs = []
    for i in range(300):
        p = rng.uniform(-1, 1, 3) * (9.0, 3.0, 9.0)
        last = p - rng.uniform(-0.4, 0.4, 3) if i % 3 == 0 else p
        objs.append((R.RT_INW_ELLIPSOID if i % 2 == 0 else R.RT_INW_CUBOID, p, last, rng.uniform(-90, 90, 3),
                     rng.uniform(0.3, 2.0, 3), MATS[i % 4], rng.uniform(0.2, 1.0, 3)))
    return _pack(objs)


def scene_one():
    z = np.zeros(3)
    return _pack([(R.RT_INW_ELLIPSOID, (0.3, 0.1, -0.2), (0.2, 0.1, -0.1), z, (1.1, 1.1, 1.1), FROSTED, (0.8, 0.6, 0.4))])


def _preset(preset, seed=0, n_hint=0, max_bounces=8):
    sc = R.make_scene(preset, seed, n_hint, spp=P.SPP)
    return SimpleNamespace(geom=sc.geom, aabbs=sc.aabbs, nodes=sc.nodes, layout=sc.layout,
                           lights=np.ascontiguousarray(sc.lights, np.float32).reshape(-1, 7), n_lights=sc.n_lights,
                           textures=None, spp=P.SPP, max_bounces=max_bounces, camera=sc.camera)


def scene_refset_tex():
    fx = _preset(R.PRESET_INW04_REFSET)
    rng = np.random.default_rng(671)
    fx.geom[0, 27], fx.geom[2 % len(fx.geom), 27] = 1.0, 2.0  # texture_index of two objects
    fx.textures = [rng.integers(0, 256, (4, 12, 3)).astype(np.uint8), rng.integers(0, 256, (5, 18, 4)).astype(np.uint8)]
    return fx


def scene_cam_random600():
    sc = R.make_scene(R.PRESET_INW01_RANDOM, 1234, 600, spp=P.SPP)
    return SimpleNamespace(geom=sc.geom, aabbs=sc.aabbs, nodes=sc.nodes, layout=1, lights=np.zeros((0, 7), np.float32),
                           n_lights=0, textures=None, spp=P.SPP, max_bounces=int(sc.params.max_bounces),
                           camera=sc.camera)


SCENES = {
    "glass600": scene_glass600,
    "glass600_b": lambda: scene_glass600(shift=True),
    "pile100": scene_pile100,
    "mixed300": scene_mixed300,
    "one": scene_one,
    "cornell": lambda: _preset(R.PRESET_INW04_CORNELL),
    "refset_tex": scene_refset_tex,
    "cam_random600": scene_cam_random600,
    "cam_cornell": lambda: _preset(R.PRESET_INW04_CORNELL, max_bounces=8),
}
SEEDS = {name: 700 + i for i, name in enumerate(SCENES)}


def kind_rays(fx, seed, n=Q):
    """The eight ray kinds of the trace fixtures, samples cycling 0..15; pad holds arbitrary bits."""
    t = make_rays(fx.geom, fx.aabbs, seed, n)
    rays = np.zeros(n, P.RAY_DTYPE)
    rays["o"], rays["d"] = t["o"], t["d"]
    rays["sample"] = np.arange(n, dtype=np.uint32) % P.SPP
    rays["pad"] = np.random.default_rng(seed).integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    return rays


def half_camera_rays(lib, fx, seed):
    """Layout-4 rooms: rays aimed from a shell outside mostly hit the outside, so every second block of
    16 queries is the 16 samples of a pixel of the preset camera's 8 x 8 frame."""
    rays = kind_rays(fx, seed)
    cam = P.camera_rays(lib, fx.camera, 8, 8, P.SPP).reshape(64, P.SPP)
    blocks = rays.reshape(-1, P.SPP)
    blocks[1::2] = cam
    return blocks.reshape(-1)


def main():
    only = set(sys.argv[1:])
    seen = dict(drops=0, nans=0, shadow=0, spread=0)
    with tempfile.TemporaryDirectory() as tmp:
        lib = P.build(tmp)
        for name in P.SCENES:
            if only and name not in only:
                continue
            fx = SCENES[name]()
            if name in P.CAM:
                rays = P.camera_rays(lib, fx.camera, P.CAM_W, P.CAM_H, P.SPP)
            elif fx.layout == 4:
                rays = half_camera_rays(lib, fx, SEEDS[name])
            else:
                rays = kind_rays(fx, SEEDS[name])
            out = {"geom": fx.geom, "aabbs": fx.aabbs, "nodes": fx.nodes, "layout": np.int32(fx.layout),
                   "lights": fx.lights, "n_tex": np.int32(len(fx.textures or [])), "spp": np.int32(fx.spp),
                   "max_bounces": np.int32(fx.max_bounces), "rays": rays.view(np.uint32).reshape(-1, 8)}
            for i, t in enumerate(fx.textures or []):
                out[f"tex{i}"] = t
            if name in P.CAM:
                out["camera"] = np.frombuffer(bytes(P.camera_of(fx.camera)), np.float32).copy()
            for inv in (0, 1):
                o, ctr = P.run(lib, fx, rays, inv)
                out[f"out{inv}"] = o.view(np.uint32).reshape(-1, 8)
                out[f"ctr{inv}"] = ctr
                # the conditions the GPU tests rely on, on the reference alone
                assert ctr[0] <= 1_000_000, (name, inv, "segments", int(ctr[0]))
                assert np.isfinite(o["rgb"]).all(), (name, inv, "non-finite rgb")
                assert not o["status"].any() and int(o["segments"].sum()) == int(ctr[0])
                seen["drops"] += int(ctr[4]); seen["nans"] += int(ctr[5]); seen["shadow"] += int(ctr[3])
                seen["spread"] += int(o["segments"].max() >= 100 and o["segments"].min() == 1)
            path = os.path.join(HERE, f"paths_{name}.npz")
            np.savez_compressed(path, **out)
            o0, o1 = out["out0"].view(P.OUT_DTYPE).reshape(-1), out["out1"].view(P.OUT_DTYPE).reshape(-1)
            print(name, "n", len(fx.geom), "queries", len(rays), "segments", int(out["ctr0"][0]), int(out["ctr1"][0]),
                  "longest", int(o0["segments"].max()), int(o1["segments"].max()),
                  "paths > 1 segment", round(float((o0["segments"] > 1).mean()), 3),
                  "shadow", int(out["ctr0"][3]), "drops", int(out["ctr0"][4]), int(out["ctr1"][4]),
                  "queries with drops", int((o0["drops"] > 0).sum()), int((o1["drops"] > 0).sum()),
                  "nans", int(out["ctr0"][5]), int(out["ctr1"][5]), "bytes", os.path.getsize(path))
            assert os.path.getsize(path) < 400_000, (name, os.path.getsize(path))
    if not only:
        assert seen["drops"] > 0, "no (fixture, order) drops a push"
        assert seen["nans"] > 0, "no fixture has a NaN direction"
        assert seen["shadow"] > 0, "no fixture casts shadow rays"
        assert seen["spread"] > 0, "no fixture has paths of >= 100 segments next to 1-segment paths"


if __name__ == "__main__":
    main()
