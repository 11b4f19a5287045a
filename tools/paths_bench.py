"""Rate of the path-query kernel (rt_path_rays_async, k_inw_paths) on the C3 scene.

The bench scene (In-Next-Week 01, 10k moving spheres, seed 1234, 1920x1080, 50 bounces) with the
500-entry sample tables of the bench frame, and three query sets built on the device with torch:
  camera    the camera's own sample rays (formed as the shader's prologue forms them, in float32
            torch arithmetic), --samples sample indices spread over the table per pixel; a wave's
            64 queries are the pixels of an 8x8 block at one sample, as in the render kernels;
  shuffled  the same set in a random order (incoherent lanes, every path length in every wave);
  reflect   first reflections off the primary hits (rt_trace_rays_async finds them): origin = hit
            point + 1e-4 n, direction = the reflection about n, the primary's sample index.
Each set is warmed up, then timed over --reps launches with HIP events (median).  Each set is also
answered once on a scene built with inw_wide_walk = 0 (the reference's LBVH walks) and must give
bit-identical outputs: an exactness check at workload size that needs no CPU reference.

Prints one JSON line (and writes it to --out).  Needs an MI355X.
    python tools/paths_bench.py [--reps 20] [--out profiles/paths_c3.json]
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

FAR = 32000.0


def dev_scene(lib, sc):
    s = lib.rt_dev_scene_inw(R.fptr(sc.geom), sc.n, sc.layout, R.fptr(sc.nodes), None, 0, sc.params.spp, 0)
    if not s:
        raise RuntimeError("rt_dev_scene_inw failed")
    return s


def cross(a, b):
    return torch.linalg.cross(a, b)


def unit(v):
    return v / v.norm(dim=-1, keepdim=True)


def camera_rays(sc, samples, dev):
    """(N, 8) float32 rt_path_ray records (sample index as bits in column 3): out_Pixel's camera ray
    (01_BVH...glsl:366-410) of `samples` sample indices per pixel; 8x8 pixel blocks, per block
    sample-major."""
    p, cam = sc.params, sc.camera
    W, H, spp = p.width // 8 * 8, p.height // 8 * 8, p.spp
    sf = torch.from_numpy(R.sample_tables(spp)[0]).to(dev)  # (spp, 2)
    D = torch.tensor(list(cam.dir), dtype=torch.float32, device=dev)
    up = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float32, device=dev)
    co = torch.tensor(list(cam.pos), dtype=torch.float32, device=dev)
    cr = cross(D, up)
    cu = cross(cr, D)
    sd = 1.0 / (2.0 * math.tan(cam.fov_y_rad * 0.5))
    ys, xs = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    blk = lambda a: a.reshape(H // 8, 8, W // 8, 8).permute(0, 2, 1, 3).reshape(-1, 1, 64)  # noqa: E731
    s_idx = (torch.arange(samples, device=dev) * spp) // samples
    xs = blk(xs).expand(-1, samples, -1).reshape(-1).float()
    ys = blk(ys).expand(-1, samples, -1).reshape(-1).float()
    s = s_idx[None, :, None].expand(W * H // 64, -1, 64).reshape(-1)
    srx = (xs / W - 0.5) * (W / H)
    sry = ys / H - 0.5
    cd = unit(D[None, :] * sd + cr[None, :] * srx[:, None] + cu[None, :] * sry[:, None])
    ox = sf[s, 0] * (cam.aperture * 0.5)
    oy = sf[s, 1] * (cam.aperture * 0.5)
    rr = cross(cd, up[None, :].expand_as(cd))
    ru = cross(rr, cd)
    tip = co[None, :] + cd + rr * ox[:, None] + ru * oy[:, None]
    la = unit(co[None, :] + cd * cam.focus_dist - tip)
    rays = torch.zeros((xs.numel(), 8), dtype=torch.float32, device=dev)
    rays[:, 0:3] = tip - la
    rays[:, 4:7] = la
    rays.view(torch.int32)[:, 3] = s.int()
    return rays


def reflect_rays(lib, scene, rays, spp, flags):
    """First reflections off the primary hits, in the primary rays' order."""
    q = rays.clone()
    q[:, 3] = FAR
    q[:, 7] = rays.view(torch.int32)[:, 3].float() * (1.0 / spp)
    hits = torch.empty_like(q)
    rc = lib.rt_trace_rays_async(scene, q.data_ptr(), q.shape[0], flags, hits.data_ptr(), None,
                                 torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise RuntimeError(f"rt_trace_rays_async -> {rc}")
    hit = hits[:, 1].view(torch.int32) >= 0
    r, h = rays[hit], hits[hit]
    d, nrm, t = r[:, 4:7], h[:, 2:5], h[:, 0:1]
    out = torch.zeros_like(r)
    out[:, 0:3] = r[:, 0:3] + d * t + 1e-4 * nrm
    out[:, 4:7] = d - 2.0 * (d * nrm).sum(1, keepdim=True) * nrm
    out.view(torch.int32)[:, 3] = r.view(torch.int32)[:, 3]
    return out.contiguous()


def paths(lib, scene, rays, max_bounces, flags, ctr=None):
    out = torch.empty_like(rays)
    rc = lib.rt_path_rays_async(scene, rays.data_ptr(), rays.shape[0], max_bounces, flags, out.data_ptr(),
                                ctr.data_ptr() if ctr is not None else None, torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise RuntimeError(f"rt_path_rays_async -> {rc}")
    return out


def timed(lib, scene, rays, max_bounces, flags, reps, warm=3):
    dev = rays.device
    for _ in range(warm):
        paths(lib, scene, rays, max_bounces, flags)
    ctr = torch.zeros(6, dtype=torch.int64, device=dev)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        out = paths(lib, scene, rays, max_bounces, flags, ctr)
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    c = [int(v) // reps for v in ctr.cpu().tolist()]
    n = rays.shape[0]
    med = ms[len(ms) // 2]
    seg = out[:, 4].view(torch.int32)
    return out, {"paths": n, "segments": c[0], "ms_median": round(med, 4), "ms_min": round(ms[0], 4),
                 "ms_max": round(ms[-1], 4), "Mpaths_per_s": round(n / med / 1e3, 1),
                 "Msegments_per_s": round(c[0] / med / 1e3, 1), "segments_per_path": round(c[0] / n, 3),
                 "longest_path": int(seg.max()), "one_segment_paths": round(float((seg == 1).float().mean()), 4),
                 "node_visits_per_segment": round(c[1] / max(c[0], 1), 2),
                 "prim_tests_per_segment": round(c[2] / max(c[0], 1), 3), "stack_drops": c[4], "nan_drops": c[5],
                 "launches_timed": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--samples", type=int, default=16, help="sample indices per pixel")
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
    sc = R.make_scene(R.PRESET_INW01_RANDOM, 1234, 10_000, width=1920, height=1080, spp=500)
    mb = int(sc.params.max_bounces)
    cam_dir = np.array(list(sc.camera.dir), np.float32)
    flags = R.RT_TRACE_INVERT if float(cam_dir.sum()) > 0.0 else 0
    scene = dev_scene(lib, sc)
    with R.options(inw_wide_walk=0):
        ref_scene = dev_scene(lib, sc)
    try:
        cam = camera_rays(sc, a.samples, dev)
        shuffled = cam[torch.randperm(cam.shape[0], device=dev, generator=gen)].contiguous()
        refl = reflect_rays(lib, scene, cam, sc.params.spp, flags)
        sets, exact = {}, True
        for name, rays in (("camera", cam), ("shuffled", shuffled), ("reflect", refl)):
            out, row = timed(lib, scene, rays, mb, flags, a.reps)
            ref = paths(lib, ref_scene, rays, mb, flags)
            torch.cuda.synchronize()
            row["bit_identical_to_lbvh_walk"] = bool(torch.equal(out.view(torch.int32), ref.view(torch.int32)))
            exact = exact and row["bit_identical_to_lbvh_walk"]
            sets[name] = row
            del out, ref
    finally:
        lib.rt_dev_scene_free(scene)
        lib.rt_dev_scene_free(ref_scene)
    res = {"tool": "tools/paths_bench.py", "scene": "C3: In-Next-Week 01, 10k moving spheres (seed 1234)",
           "objects": sc.n, "flags": flags, "table_spp": sc.params.spp, "max_bounces": mb,
           "samples_per_pixel": a.samples, "sets": sets,
           "kernel": {"name": "k_inw_paths<false, true>", **R.paths_kernel_info(False, True)},
           "options": "defaults", "timing": "HIP events around each launch, median of the timed launches"}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    if not exact:
        raise SystemExit("outputs differ from the LBVH walk's")


if __name__ == "__main__":
    main()
