"""Rate of the IOW-03 path-query kernel (rt_path_iow_rays_async, k_iow_paths) on the C2 scene.

The bench scene (In-One-Weekend 03, the final scene, seed 20250131, the preset's frame, 50 bounces)
with the 100-entry sample tables of the bench frame, and four query sets built on the device with
torch:
  camera_chains  the camera's own sample rays (formed as out_Pixel forms them, in float32 torch
                 arithmetic) of --blocks 8x8 pixel blocks spread evenly over the frame (the whole
                 frame at 50 bounces is minutes of the linear loop the sets are checked against),
                 --samples sample indices spread over the table per pixel, each pixel's
                 samples a chain in sample order, zero incoming state; consecutive chains are the
                 pixels of an 8x8 block, so a wave's 64 lanes hold one block as in the render kernels;
  camera_single  the same rays at chain = 1: every query independent, zero state;
  shuffled       the chains of camera_chains in a random order (incoherent lanes);
  reflect        first reflections off the primary hits (rt_trace_iow_rays_async finds them): origin =
                 hit point + 1e-4 n, direction = the reflection about n, the primary's sample index,
                 chain = 1, zero state.
Every set runs at the frame's 50 bounces and at --short-bounces: at 50 a few paths are tens of thousands
of segments long (one lane, alone, for the rest of the launch), at 8 none is; the 8-bounce sets take
--short-blocks pixel blocks, so that a launch outlasts its longest chain.
Each set is warmed up, then timed over --reps launches with HIP events (median).  Each set is also
answered once on a scene built with iow_linear = 1 (the reference's loop over every object) and must
give bit-identical outputs: an exactness check at workload size that needs no CPU reference.

Prints one JSON line (and writes it to --out).  Needs an MI355X.
    python tools/path_iow_bench.py [--reps 20] [--out profiles/path_iow_c2.json]
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "raytracing-tests_amd")]

import torch  # noqa: E402

import rt_amd as R  # noqa: E402

FAR = 32000.0


def dev_scene(lib, sc):
    s = lib.rt_dev_scene_iow03(R.fptr(sc.types), R.fptr(sc.records), sc.n, sc.params.spp, 0)
    if not s:
        raise RuntimeError("rt_dev_scene_iow03 failed")
    return s


def cross(a, b):
    return torch.linalg.cross(a, b)


def unit(v):
    return v / v.norm(dim=-1, keepdim=True)


def camera_rays(sc, samples, blocks, dev):
    """(pixels, samples, 12) float32 rt_path_iow_ray records (sample index as bits in column 3, ri_in 0):
    out_Pixel's camera ray (03...glsl:362-410) of `samples` sample indices per pixel; pixels in 8x8
    blocks, `blocks` of them spread evenly over the frame's."""
    p, cam = sc.params, sc.camera
    W, H, spp = p.width // 8 * 8, p.height // 8 * 8, p.spp
    sf, _, ring = R.sample_tables(spp)
    sf, ring = torch.from_numpy(sf).to(dev), torch.from_numpy(ring).to(dev).float()
    D = torch.tensor(list(cam.dir), dtype=torch.float32, device=dev)
    up = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float32, device=dev)
    P = torch.tensor(list(cam.pos), dtype=torch.float32, device=dev)
    cr = cross(D, up)
    cu = cross(cr, D)
    sd = 1.0 / (2.0 * math.tan(cam.fov_y_rad * 0.5))
    grid = math.ceil(math.sqrt(spp))
    aspect = p.width / p.height
    ys, xs = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    total = (H // 8) * (W // 8)
    blocks = min(blocks, total)
    pick = (torch.arange(blocks, device=dev) * total) // blocks
    blk = lambda a: a.reshape(H // 8, 8, W // 8, 8).permute(0, 2, 1, 3).reshape(total, 64)[pick].reshape(-1, 1)  # noqa: E731
    s_idx = (torch.arange(samples, device=dev) * spp) // samples
    xs = blk(xs).expand(-1, samples).reshape(-1).float()
    ys = blk(ys).expand(-1, samples).reshape(-1).float()
    s = s_idx[None, :].expand(blocks * 64, -1).reshape(-1)
    sx = aspect * (xs * 2.0 - p.width) / (2.0 * p.width) + aspect / (p.width * grid) * ring[s, 0]
    sy = (ys * 2.0 - p.height) / (2.0 * p.height) + 1.0 / (p.height * grid) * ring[s, 1]
    ro = P[None, :] + cr[None, :] * (sf[s, 0] * cam.aperture * 0.5)[:, None] + \
        cu[None, :] * (sf[s, 1] * cam.aperture * 0.5)[:, None]
    ld = unit(P[None, :] + D[None, :] * cam.focus_dist - ro)
    r_ = cross(ld, up[None, :].expand_as(ld))
    u_ = cross(cr[None, :].expand_as(ld), ld)
    rd = unit(ld * sd + r_ * sx[:, None] + u_ * sy[:, None])
    rays = torch.zeros((xs.numel(), 12), dtype=torch.float32, device=dev)
    rays[:, 0:3] = ro
    rays[:, 4:7] = rd
    rays.view(torch.int32)[:, 3] = s.int()
    return rays.reshape(blocks * 64, samples, 12)


def reflect_rays(lib, scene, rays):
    """First reflections off the primary hits, in the primary rays' order."""
    q = rays[:, 0:8].contiguous()
    q[:, 3] = FAR
    q[:, 7] = 0.0
    hits = torch.empty_like(q)
    rc = lib.rt_trace_iow_rays_async(scene, q.data_ptr(), q.shape[0], 0, hits.data_ptr(), None,
                                     torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise RuntimeError(f"rt_trace_iow_rays_async -> {rc}")
    hit = hits[:, 1].view(torch.int32) >= 0
    r, h = rays[hit], hits[hit]
    d, nrm, t = r[:, 4:7], h[:, 2:5], h[:, 0:1]
    out = torch.zeros_like(r)
    out[:, 0:3] = r[:, 0:3] + d * t + 1e-4 * nrm
    out[:, 4:7] = unit(d - 2.0 * (d * nrm).sum(1, keepdim=True) * nrm)
    out.view(torch.int32)[:, 3] = r.view(torch.int32)[:, 3]
    return out.contiguous()


def paths(lib, scene, rays, chain, max_bounces, ctr=None):
    out = torch.empty_like(rays)
    rc = lib.rt_path_iow_rays_async(scene, rays.data_ptr(), rays.shape[0], chain, max_bounces, 0, out.data_ptr(),
                                    ctr.data_ptr() if ctr is not None else None,
                                    torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise RuntimeError(f"rt_path_iow_rays_async -> {rc}")
    return out


def timed(lib, scene, rays, chain, max_bounces, reps, warm=3):
    dev = rays.device
    for _ in range(warm):
        paths(lib, scene, rays, chain, max_bounces)
    ctr = torch.zeros(6, dtype=torch.int64, device=dev)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        out = paths(lib, scene, rays, chain, max_bounces, ctr)
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    c = [int(v) // reps for v in ctr.cpu().tolist()]
    n = rays.shape[0]
    med = ms[len(ms) // 2]
    seg = out[:, 4].view(torch.int32)
    stale = out[:, 3].view(torch.int32)
    per_chain = torch.nn.functional.pad(seg.long(), (0, -n % chain)).reshape(-1, chain).sum(1)
    return out, {"paths": n, "chain": chain, "segments": c[0], "ms_median": round(med, 4), "ms_min": round(ms[0], 4),
                 "ms_max": round(ms[-1], 4), "Mpaths_per_s": round(n / med / 1e3, 2),
                 "Msegments_per_s": round(c[0] / med / 1e3, 1), "segments_per_path": round(c[0] / n, 3),
                 "longest_path": int(seg.max()), "longest_chain_segments": int(per_chain.max()),
                 "us_per_segment_of_longest_chain": round(med * 1e3 / int(per_chain.max()), 3),
                 "one_segment_paths": round(float((seg == 1).float().mean()), 4),
                 "stale_paths": round(float((stale != 0).float().mean()), 4),
                 "node_visits_per_segment": round(c[1] / max(c[0], 1), 2),
                 "prim_tests_per_segment": round(c[2] / max(c[0], 1), 3), "stack_drops": c[4], "nan_drops": c[5],
                 "launches_timed": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--samples", type=int, default=16, help="sample indices per pixel")
    ap.add_argument("--blocks", type=int, default=1024, help="8x8 pixel blocks, spread evenly over the frame")
    ap.add_argument("--short-bounces", type=int, default=8, help="the second bounce limit every set runs at")
    ap.add_argument("--short-blocks", type=int, default=8192, help="... and its 8x8 pixel blocks")
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
    sc = R.make_scene(R.PRESET_IOW03_FINAL, 20250131, 0)
    mb = int(sc.params.max_bounces)
    scene = dev_scene(lib, sc)
    with R.options(iow_linear=1):
        ref_scene = dev_scene(lib, sc)
    try:
        def query_sets(blocks):
            cam = camera_rays(sc, a.samples, blocks, dev)
            flat = cam.reshape(-1, 12).contiguous()
            shuffled = cam[torch.randperm(cam.shape[0], device=dev, generator=gen)].reshape(-1, 12).contiguous()
            return (("camera_chains", flat, a.samples), ("camera_single", flat, 1), ("shuffled", shuffled, a.samples),
                    ("reflect", reflect_rays(lib, scene, flat), 1))

        sets, exact = {}, True
        # at the frame's bounce limit a launch lasts as long as its longest chain, one lane running alone;
        # at --short-bounces no path is long, and with --short-blocks blocks the launch outlasts its longest
        # chain, so the rate is the segment body's
        for mb_set, blocks in ((mb, a.blocks), (a.short_bounces, a.short_blocks)):
            rows = {"pixel_blocks": min(blocks, (sc.params.width // 8) * (sc.params.height // 8))}
            for name, rays, chain in query_sets(blocks):
                out, row = timed(lib, scene, rays, chain, mb_set, a.reps)
                ref = paths(lib, ref_scene, rays, chain, mb_set)
                torch.cuda.synchronize()
                row["bit_identical_to_linear_loop"] = bool(torch.equal(out.view(torch.int32), ref.view(torch.int32)))
                exact = exact and row["bit_identical_to_linear_loop"]
                rows[name] = row
                del out, ref, rays
            sets[f"max_bounces_{mb_set}"] = rows
    finally:
        lib.rt_dev_scene_free(scene)
        lib.rt_dev_scene_free(ref_scene)
    res = {"tool": "tools/path_iow_bench.py", "scene": "C2: In-One-Weekend 03, final scene (seed 20250131)",
           "objects": sc.n, "width": int(sc.params.width), "height": int(sc.params.height),
           "table_spp": int(sc.params.spp), "max_bounces": [mb, a.short_bounces],
           "samples_per_pixel": a.samples, "sets": sets,
           "kernel": {"name": "k_iow_paths<true>", **R.path_iow_kernel_info(True)},
           "options": "defaults", "timing": "HIP events around each launch, median of the timed launches"}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    if not exact:
        raise SystemExit("outputs differ from the linear loop's")


if __name__ == "__main__":
    main()
