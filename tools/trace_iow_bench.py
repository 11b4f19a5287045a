"""Rate of the standalone IOW-03 closest-hit kernel (rt_trace_iow_rays_async, k_iow_trace) on the
C2 scene: the LDS-staged 4-wide walk of k_iow03sL with no speculation records, ray stack or resolve
around it.

Three query sets on the bench scene (In-One-Weekend 03 final scene, seed 20250131, 1200x800), built
on the device with torch (the ray builders are tools/trace_bench.py's):
  primary   camera-like rays, 8x8 pixel blocks in order (neighbouring lanes, neighbouring pixels);
  bounce    first reflections off the primary hits: origin = hit point + 1e-4 n, direction = the
            reflection about n, in the primary rays' order;
  shuffled  the bounce set in a random order (incoherent lanes).
The sets grow (samples per pixel double) until a primary launch takes at least --min-ms.  Each set
is warmed up, then timed over --reps launches with HIP events.  Each set is also traced once on a
scene built with iow_linear = 1 (the reference's linear loop) and must give bit-identical hits: an
exactness check at workload size that needs no CPU reference.

Prints one JSON line (and writes it to --out).  Needs an MI355X.
    python tools/trace_iow_bench.py [--reps 20] [--out profiles/trace_iow_c2.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "raytracing-tests_amd"), os.path.join(ROOT, "tools")]

import torch  # noqa: E402

import rt_amd as R  # noqa: E402
from trace_bench import bounce_rays, primary_rays  # noqa: E402


def dev_scene(lib, sc):
    s = lib.rt_dev_scene_iow03(R.fptr(sc.types), R.fptr(sc.records), sc.n, 1, 0)
    if not s:
        raise RuntimeError("rt_dev_scene_iow03 failed")
    return s


def trace(lib, scene, rays, ctr=None):
    hits = torch.empty_like(rays)
    rc = lib.rt_trace_iow_rays_async(scene, rays.data_ptr(), rays.shape[0], 0, hits.data_ptr(),
                                     ctr.data_ptr() if ctr is not None else None,
                                     torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise RuntimeError(f"rt_trace_iow_rays_async -> {rc}")
    return hits


def timed(lib, scene, rays, reps, warm=3):
    dev = rays.device
    for _ in range(warm):
        trace(lib, scene, rays)
    ctr = torch.zeros(6, dtype=torch.int64, device=dev)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        hits = trace(lib, scene, rays, ctr)
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    c = [int(v) // reps for v in ctr.cpu().tolist()]
    n = rays.shape[0]
    med = ms[len(ms) // 2]
    return hits, {"rays": n, "ms_median": round(med, 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4),
                  "Mqueries_per_s": round(n / med / 1e3, 1), "hit_fraction": None,
                  "node_visits_per_query": round(c[1] / n, 2), "prim_tests_per_query": round(c[2] / n, 3),
                  "launches_timed": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--samples", type=int, default=16, help="primary rays per pixel to start from")
    ap.add_argument("--min-ms", type=float, default=3.0, help="a primary launch takes at least this long")
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
    sc = R.make_scene(R.PRESET_IOW03_FINAL, 20250131, 0, width=1200, height=800)
    scene = dev_scene(lib, sc)
    with R.options(iow_linear=1):
        ref_scene = dev_scene(lib, sc)
    try:
        samples = a.samples
        while True:
            prim = primary_rays(sc, samples, dev, gen)
            _, row = timed(lib, scene, prim, 3, warm=1)
            if row["ms_median"] >= a.min_ms or samples >= 128:
                break
            samples *= 2
        bounce = bounce_rays(prim, trace(lib, scene, prim))
        shuffled = bounce[torch.randperm(bounce.shape[0], device=dev, generator=gen)].contiguous()
        sets, exact = {}, True
        for name, rays in (("primary", prim), ("bounce", bounce), ("shuffled", shuffled)):
            hits, row = timed(lib, scene, rays, a.reps)
            row["hit_fraction"] = round(float((hits[:, 1].view(torch.int32) >= 0).float().mean()), 4)
            ref = trace(lib, ref_scene, rays)
            torch.cuda.synchronize()
            row["bit_identical_to_linear_loop"] = bool(torch.equal(hits.view(torch.int32), ref.view(torch.int32)))
            exact = exact and row["bit_identical_to_linear_loop"]
            sets[name] = row
            del hits, ref
    finally:
        lib.rt_dev_scene_free(scene)
        lib.rt_dev_scene_free(ref_scene)
    nodes = R.iow_host_build(sc.types, sc.records, sc.n)["wide_nodes"]
    res = {"tool": "tools/trace_iow_bench.py", "scene": "C2: In-One-Weekend 03 final scene (seed 20250131), 1200x800",
           "objects": sc.n, "wide_nodes": nodes, "samples_per_pixel": samples, "sets": sets,
           "kernel": {"name": "k_iow_trace<false, true>", **R.trace_iow_kernel_info(False, True)},
           "kernel_global_nodes": {"name": "k_iow_trace<false, false>", **R.trace_iow_kernel_info(False, False)},
           "options": "defaults", "timing": "HIP events around each launch, median of the timed launches"}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    if not exact:
        raise SystemExit("hits differ from the linear loop's")


if __name__ == "__main__":
    main()
