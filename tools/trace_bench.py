"""Rate of the standalone closest-hit kernel (rt_trace_rays_async, k_inw_trace) on the C3 scene.

VERDICT's step-one measurement: the walk alone -- its natural registers, no pending-ray stack, no
fold -- on the rays k_inw_pm walks in its bounce round.  Three query sets of at least 4M rays on
the bench scene (In-Next-Week 01, 10k moving spheres, seed 1234), built on the device with torch:
  primary   camera-like rays, 8x8 pixel blocks in order (neighbouring lanes, neighbouring pixels);
  bounce    first-bounce rays from the primary hits: origin = hit point + 1e-4 n, direction =
            the reflection about n, in the primary rays' order (coherent origins);
  shuffled  the bounce set in a random order (incoherent lanes).
Each set is warmed up, then timed over --reps launches with HIP events.  Each set is also traced
once on a scene built with inw_wide_walk = 0 (the reference's LBVH walk) and must give
bit-identical hits: an exactness check at workload size that needs no CPU reference.

Prints one JSON line (and writes it to --out).  Needs an MI355X.
    python tools/trace_bench.py [--reps 20] [--out profiles/trace_c3.json]
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "raytracing-tests_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import rt_amd as R  # noqa: E402

MIN_RAYS = 4_000_000
FAR = 32000.0


def dev_scene(lib, sc):
    s = lib.rt_dev_scene_inw(R.fptr(sc.geom), sc.n, sc.layout, R.fptr(sc.nodes), None, 0, 1, 0)
    if not s:
        raise RuntimeError("rt_dev_scene_inw failed")
    return s


def primary_rays(sc, samples, dev, gen):
    """(N, 8) float32 rt_ray records: a pinhole camera at the scene's, `samples` jittered rays per
    pixel with time ratios s / samples, pixels in 8x8 blocks."""
    p, cam = sc.params, sc.camera
    W, H = p.width // 8 * 8, p.height // 8 * 8
    f = torch.tensor(list(cam.dir), dtype=torch.float64)
    f = f / f.norm()
    right = torch.linalg.cross(f, torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64))
    right = right / right.norm()
    up = torch.linalg.cross(right, f)
    sd = 1.0 / (2.0 * math.tan(cam.fov_y_rad * 0.5))
    ys, xs = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    blk = lambda a: a.reshape(H // 8, 8, W // 8, 8).permute(0, 2, 1, 3).reshape(-1)  # noqa: E731
    xs, ys = blk(xs), blk(ys)
    xs = xs[:, None].expand(-1, samples).reshape(-1).float()
    ys = ys[:, None].expand(-1, samples).reshape(-1).float()
    n = xs.numel()
    jx, jy = torch.rand(n, device=dev, generator=gen), torch.rand(n, device=dev, generator=gen)
    sx = ((xs + jx) / W - 0.5) * (W / H)
    sy = (ys + jy) / H - 0.5
    f, right, up = (v.float().to(dev) for v in (f, right, up))
    d = f[None, :] * sd + right[None, :] * sx[:, None] + up[None, :] * sy[:, None]
    d = d / d.norm(dim=1, keepdim=True)
    rays = torch.empty((n, 8), dtype=torch.float32, device=dev)
    rays[:, 0:3] = torch.tensor(list(cam.pos), dtype=torch.float32, device=dev)
    rays[:, 3] = FAR
    rays[:, 4:7] = d
    rays[:, 7] = (torch.arange(n, device=dev) % samples).float() / samples
    return rays


def bounce_rays(rays, hits):
    """First-bounce rays of the primary hits, in the primary rays' order."""
    hit = hits[:, 1].view(torch.int32) >= 0
    r, h = rays[hit], hits[hit]
    d, nrm, t = r[:, 4:7], h[:, 2:5], h[:, 0:1]
    out = torch.empty_like(r)
    out[:, 0:3] = r[:, 0:3] + d * t + 1e-4 * nrm
    out[:, 3] = FAR
    out[:, 4:7] = d - 2.0 * (d * nrm).sum(1, keepdim=True) * nrm
    out[:, 7] = r[:, 7]
    return out.contiguous()


def trace(lib, scene, rays, flags, ctr=None):
    hits = torch.empty_like(rays)
    rc = lib.rt_trace_rays_async(scene, rays.data_ptr(), rays.shape[0], flags, hits.data_ptr(),
                                 ctr.data_ptr() if ctr is not None else None, torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise RuntimeError(f"rt_trace_rays_async -> {rc}")
    return hits


def timed(lib, scene, rays, flags, reps, warm=3):
    dev = rays.device
    for _ in range(warm):
        trace(lib, scene, rays, flags)
    ctr = torch.zeros(6, dtype=torch.int64, device=dev)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        hits = trace(lib, scene, rays, flags, ctr)
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    c = [int(v) // reps for v in ctr.cpu().tolist()]
    n = rays.shape[0]
    med = ms[len(ms) // 2]
    return hits, {"rays": n, "ms_median": round(med, 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4),
                  "Mqueries_per_s": round(n / med / 1e3, 1), "hit_fraction": None,
                  "node_visits_per_query": round(c[1] / n, 2), "prim_tests_per_query": round(c[2] / n, 3),
                  "stack_drops": c[4], "launches_timed": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--samples", type=int, default=16, help="primary rays per pixel (raised until the bounce set has 4M rays)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    lib = R.load()
    if lib.rt_device_info(0, None, 0, None) != 0:
        raise RuntimeError("no gfx950 device: the rates are measured on the GPU or not at all")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    sc = R.make_scene(R.PRESET_INW01_RANDOM, 1234, 10_000, width=1920, height=1080)
    cam_dir = np.array(list(sc.camera.dir), np.float32)
    flags = R.RT_TRACE_INVERT if float(cam_dir.sum()) > 0.0 else 0
    scene = dev_scene(lib, sc)
    with R.options(inw_wide_walk=0):
        ref_scene = dev_scene(lib, sc)
    try:
        samples = a.samples
        while True:
            prim = primary_rays(sc, samples, dev, gen)
            bounce = bounce_rays(prim, trace(lib, scene, prim, flags))
            if prim.shape[0] >= MIN_RAYS and bounce.shape[0] >= MIN_RAYS:
                break
            samples *= 2
            if samples > 64:
                raise RuntimeError("the camera sees too few objects for a 4M-ray bounce set")
        shuffled = bounce[torch.randperm(bounce.shape[0], device=dev, generator=gen)].contiguous()
        sets, exact = {}, True
        for name, rays in (("primary", prim), ("bounce", bounce), ("shuffled", shuffled)):
            hits, row = timed(lib, scene, rays, flags, a.reps)
            row["hit_fraction"] = round(float((hits[:, 1].view(torch.int32) >= 0).float().mean()), 4)
            ref = trace(lib, ref_scene, rays, flags)
            torch.cuda.synchronize()
            row["bit_identical_to_lbvh_walk"] = bool(torch.equal(hits.view(torch.int32), ref.view(torch.int32)))
            exact = exact and row["bit_identical_to_lbvh_walk"]
            sets[name] = row
            del hits, ref
    finally:
        lib.rt_dev_scene_free(scene)
        lib.rt_dev_scene_free(ref_scene)
    res = {"tool": "tools/trace_bench.py", "scene": "C3: In-Next-Week 01, 10k moving spheres (seed 1234)",
           "objects": sc.n, "flags": flags, "samples_per_pixel": samples, "sets": sets,
           "kernel": {"name": "k_inw_trace<false, true>", **R.trace_kernel_info(False, True)},
           "kernel_any": {"name": "k_inw_trace<true, true>", **R.trace_kernel_info(True, True)},
           "options": "defaults", "timing": "HIP events around each launch, median of the timed launches"}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    if not exact:
        raise SystemExit("hits differ from the LBVH walk's")


if __name__ == "__main__":
    main()
