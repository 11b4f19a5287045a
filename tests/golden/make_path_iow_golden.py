"""Regenerate tests/golden/path_iow_*.npz: IOW-03 path queries and the reference answers of
tests/path_iow_ref.c (the CPU oracle's launch_rays per query, on a ray stack that holds the incoming RI
state).

The scenes are those of the trace_iow_*.npz fixtures (types, records); a path fixture names its scene
and holds rays (Q, 12 float32 = rt_path_iow_ray), out (Q, 12 uint32 = rt_path_iow_out), chain,
max_bounces, ctr (segments, drops, nans of the whole batch) and, for cam_final, the camera (pos3, dir3,
fov_y_rad, aperture, focus_dist).  The scatter table has 8 entries everywhere.  The generator asserts
that the sets reach the ground the feature adds: stale reads, dropped pushes, answers that depend on the
incoming state, NaN directions, a long path.  Run from the repo root (needs gcc and the built
librt_hip.so for the camera of the final scene; no GPU):
    python tests/golden/make_path_iow_golden.py
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "raytracing-tests_amd"), os.path.dirname(HERE)]

import rt_amd as R  # noqa: E402
import path_iow_ref as P  # noqa: E402
import trace_iow_ref as T  # noqa: E402

RI_VALUES = np.array([0.0, 1.0, 1.3, 1.5, 2.4], np.float32)
SCENE_OF = {"final": "final", "final_deep": "final", "rot": "rot", "ref3": "ref3", "shells": "shells", "one": "one",
            "state": "rot", "cam_final": "final"}
BOUNCES = {"final_deep": 50}
SEEDS = {name: 700 + i for i, name in enumerate(P.SETS)}


def chains(rng, origins, dirs, n_chains, length=8, sigma=0.002):
    """n_chains chains of `length`: one origin, `length` directions around one direction, samples j % 8;
    later queries carry an ri_in the chain must ignore; pad holds random bits."""
    rays = np.zeros((n_chains, length), P.RAY_DTYPE)
    for k in range(n_chains):
        d = np.asarray(dirs[k], np.float64)
        for j in range(length):
            dj = d + rng.normal(0.0, sigma, 3)
            if np.isfinite(d).all() and abs(np.linalg.norm(d) - 1.0) < 1e-3:
                dj = dj / np.linalg.norm(dj)  # near-unit seeds stay near unit (the BVH walk); odd ones stay odd
            rays[k, j]["o"], rays[k, j]["d"] = origins[k], dj.astype(np.float32)
            rays[k, j]["sample"] = j % P.SPP
            if j:
                rays[k, j]["ri_in"] = rng.choice(RI_VALUES, 4)
    rays = rays.reshape(-1)
    rays["pad"] = rng.integers(0, 2 ** 32, len(rays), dtype=np.uint64).astype(np.uint32)
    return rays


def seeds_from_trace(name, n):
    rays = T.load_fixture(name)["rays"][:n]
    return rays["o"].copy(), rays["d"].copy()


def make_set(name, rng, lib):
    """rays, chain, max_bounces, extras"""
    if name in ("final", "final_deep"):
        n = 600 if name == "final" else 64
        o = np.tile(np.array([13.0, 2.0, 3.0], np.float32), (n, 1))
        tgt = rng.uniform((-5.0, 0.0, -5.0), (5.0, 1.5, 5.0), (n, 3))
        d = tgt - o
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        return chains(rng, o, d, n), 8, BOUNCES.get(name, 8), {}
    if name in ("rot", "ref3", "shells"):
        o, d = seeds_from_trace(name, 600)
        return chains(rng, o, d, 600), 8, 8, {}
    if name == "one":
        o, d = seeds_from_trace(name, 16)
        return chains(rng, o, d, 16), 8, 8, {}
    if name == "state":
        t = T.load_fixture("rot")["rays"][:2048]  # every eighth-kind of that set: zero, NaN and non-unit directions too
        rays = np.zeros(len(t), P.RAY_DTYPE)
        rays["o"], rays["d"] = t["o"], t["d"]
        rays["sample"] = rng.integers(0, P.SPP, len(t))
        rays["ri_in"] = rng.choice(RI_VALUES[1:], (len(t), 4))
        rays["ri_in"][rng.random((len(t), 4)) < 0.1] = 0.0
        assert rays["ri_in"].any(1).all()
        bad = rng.choice(len(t), 24, replace=False)
        rays["sample"][bad] = rng.choice(np.array([8, 9, 100, 0xFFFFFFFF], np.uint32), 24)
        rays["pad"] = rng.integers(0, 2 ** 32, len(t), dtype=np.uint64).astype(np.uint32)
        return rays, 1, 8, {}
    if name == "cam_final":
        sc = R.make_scene(R.PRESET_IOW03_FINAL, 20250131, 0)
        fin = T.load_fixture("final")
        assert np.array_equal(sc.types, fin["types"]) and np.array_equal(sc.records, fin["records"])
        c = sc.camera
        cam9 = np.array([*c.pos, *c.dir, c.fov_y_rad, c.aperture, c.focus_dist], np.float32)
        rays = P.camera_rays(lib, cam9, P.CAM_W, P.CAM_H, P.SPP)
        return rays, P.SPP, int(sc.params.max_bounces), {"camera": cam9}
    raise KeyError(name)


def main():
    only = set(sys.argv[1:])
    lim = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE)
              if f.endswith(".npz") and not f.startswith("path_iow_"))
    with tempfile.TemporaryDirectory() as tmp:
        lib = P.build(tmp)
        for name in P.SETS:
            if only and name not in only:
                continue
            rng = np.random.default_rng(SEEDS[name])
            scene = T.load_fixture(SCENE_OF[name])
            types, rec = scene["types"], scene["records"]
            rays, chain, mb, extra = make_set(name, rng, lib)
            out, ctr = P.run(lib, types, rec, rays, mb, chain)
            ran = out["status"] == 0
            stale = float((out["stale"][ran] != 0).mean())
            drops = float((out["drops"][ran] > 0).mean())
            nans = int(out["nans"].sum())
            dep = -1.0
            if name in ("final", "rot"):  # the same rays, each alone with the zero state
                zero = rays.copy()
                zero["ri_in"] = 0.0
                alone, _ = P.run(lib, types, rec, zero, mb, 1)
                later = np.arange(len(rays)) % chain != 0
                dep = float((out["rgb"].view(np.uint32) != alone["rgb"].view(np.uint32)).any(1)[later].mean())
            # the floors: a test must not be able to pass on rays that never touch the new ground
            if name in ("final", "rot"):
                assert stale >= 0.05, (name, stale)
            if name == "rot":
                assert dep >= 0.05, (name, dep)
            if name == "shells":
                assert nans > 0 and drops > 0.5, (name, nans, drops)
            if name == "final_deep":
                assert out["segments"].max() > 1000, (name, int(out["segments"].max()))
            if name == "state":
                assert (out["status"] == 1).sum() == 24 and (out["stale"] != 0).mean() >= 0.05
            npz = {"scene": np.array(SCENE_OF[name]), "rays": rays.view(np.float32).reshape(-1, 12),
                   "out": out.view(np.uint32).reshape(-1, 12), "chain": np.int64(chain), "max_bounces": np.int64(mb),
                   "ctr": ctr, **extra}
            path = os.path.join(HERE, f"path_iow_{name}.npz")
            np.savez_compressed(path, **npz)
            assert os.path.getsize(path) <= lim, (name, os.path.getsize(path), lim)
            print(name, "queries", len(rays), "chain", chain, "bounces", mb, "stale", round(stale, 3), "drops",
                  round(drops, 3), "nans", nans, "state-dependent", round(dep, 3), "longest",
                  int(out["segments"].max()), "segments", int(ctr[0]), "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
