"""Rates of the pixel-query kernels (rt_camera_rays_async: k_camera_rays; rt_pixel_query_async: the
rays, the unchanged path kernel, k_pixel_fold) on the C3 scene.

The bench scene (In-Next-Week 01, 10k moving spheres, seed 1234, 1920x1080, 50 bounces) with the
500-entry sample tables of the bench frame.  Two measurements, each warmed up and then timed over --reps
launches with HIP events (median, min and max reported):
  camera_rays  rt_camera_rays_async for the set tools/paths_bench.py calls "camera" -- every pixel of the
               frame in 8x8 blocks -- and --samples contiguous sample indices per pixel (33.2 M records of
               32 B at the default 16).  Beside it, in the same process: a hipMemsetAsync of the same byte
               count (the fill rate the store-bound kernel is compared with) and rt_path_rays_async alone
               on the rays the call produced.
  pixel_query  rt_pixel_query_async for a --block x --block pixel block at the frame's centre and all
               500 samples.  Beside it: its camera-ray step alone and the path kernel alone on the same
               rays.  k_pixel_fold has no entry point of its own: its share is the whole query minus
               those two (a `rocprofv3 --kernel-trace --stats` run of this script gives its kernel time
               directly).
Checks at workload size, no CPU reference needed: the 16-sample rays equal the first 16 of each pixel's
500-sample rays, and the query's pixels equal rt_render_image_async's pixels of that block's tile.

Prints one JSON line (and writes it to --out).  Needs an MI355X.
    python tools/pixels_bench.py [--reps 20] [--out profiles/pixels_c3.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "raytracing-tests_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import rt_amd as R  # noqa: E402


def hip_runtime():
    """The HIP runtime this process has loaded (torch's and librt_hip.so's: one copy), for hipMemsetAsync.
    It is opened by the path it is mapped from, so streams and pointers are that runtime's own."""
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64.so" in line})
    if len(paths) != 1:
        raise RuntimeError(f"expected one loaded HIP runtime, found {paths}")
    lib = C.CDLL(paths[0])
    lib.hipMemsetAsync.restype = C.c_int
    lib.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    return lib


def block_pixels(w, h):
    """Every pixel of the w x h frame (multiples of 8) as (x, y) int32 pairs, 8x8 blocks row-major, each
    block row-major: the order of paths_bench.py's camera set."""
    ys, xs = np.meshgrid(np.arange(h, dtype=np.int32), np.arange(w, dtype=np.int32), indexing="ij")
    blk = lambda a: a.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3).reshape(-1)  # noqa: E731
    return np.stack([blk(xs), blk(ys)], axis=1)


def timed(fn, reps, warm=3):
    """fn() enqueued on the current stream: {ms_median, ms_min, ms_max} over reps launches after warm."""
    for _ in range(warm):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return {"ms_median": round(ms[len(ms) // 2], 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4)}


def ok(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} -> {rc}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--samples", type=int, default=16, help="contiguous sample indices per pixel (camera_rays)")
    ap.add_argument("--block", type=int, default=64, help="side of the pixel block (pixel_query)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    lib = R.load()
    if lib.rt_device_info(0, None, 0, None) != 0:
        raise RuntimeError("no gfx950 device: the rates are measured on the GPU or not at all")
    hip = hip_runtime()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    stream = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
    sc = R.make_scene(R.PRESET_INW01_RANDOM, 1234, 10_000, width=1920, height=1080, spp=500)
    p, cam = sc.params, sc.camera
    spp, mb = int(p.spp), int(p.max_bounces)
    d = np.array(list(cam.dir), np.float32)
    flags = R.RT_TRACE_INVERT if np.float32(np.float32(d[0] + d[1]) + d[2]) > 0 else 0
    scene = R.dev_scene(sc, device=0)
    res = {}
    try:
        # ---- camera rays of the whole frame
        px = block_pixels(p.width // 8 * 8, p.height // 8 * 8)
        d_px = torch.from_numpy(px.copy()).to(dev)
        n = len(px) * a.samples
        d_rays = torch.empty((n, 8), dtype=torch.float32, device=dev)
        d_out = torch.empty_like(d_rays)
        nbytes = n * 32

        def rays():
            ok(lib.rt_camera_rays_async(scene, C.byref(cam), C.byref(p), d_px.data_ptr(), len(px), 0, a.samples,
                                        d_rays.data_ptr(), stream()), "rt_camera_rays_async")

        def fill():
            ok(hip.hipMemsetAsync(d_out.data_ptr(), 0, nbytes, stream()), "hipMemsetAsync")

        def paths():
            ok(lib.rt_path_rays_async(scene, d_rays.data_ptr(), n, mb, flags, d_out.data_ptr(), None, stream()),
               "rt_path_rays_async")

        t_rays, t_fill = timed(rays, a.reps), timed(fill, a.reps)
        t_rays2, t_fill2 = timed(rays, a.reps), timed(fill, a.reps)  # again, alternating: the spread
        t_paths = timed(paths, a.reps)
        gbs = lambda t: round(nbytes / t["ms_median"] / 1e6, 1)  # noqa: E731
        res["camera_rays"] = {
            "pixels": len(px), "samples": a.samples, "records": n, "bytes_written": nbytes,
            "k_camera_rays": {**t_rays, "GB_per_s": gbs(t_rays), "again": {**t_rays2, "GB_per_s": gbs(t_rays2)}},
            "hipMemsetAsync_same_bytes": {**t_fill, "GB_per_s": gbs(t_fill),
                                          "again": {**t_fill2, "GB_per_s": gbs(t_fill2)}},
            "share_of_fill_rate": round(t_fill["ms_median"] / t_rays["ms_median"], 3),
            "rt_path_rays_async_on_these_rays": {**t_paths, "Mpaths_per_s": round(n / t_paths["ms_median"] / 1e3, 1)}}
        first = d_rays.view(torch.int32).reshape(len(px), a.samples, 8)[:4096].clone()
        del d_rays, d_out

        # ---- the pixel query of one block
        b = a.block
        x0, y0 = (p.width - b) // 2 // 8 * 8, (p.height - b) // 2 // 8 * 8
        qpx = np.array([(x0 + x, y0 + y) for y in range(b) for x in range(b)], np.int32)
        d_qpx = torch.from_numpy(qpx).to(dev)
        nq = len(qpx) * spp
        need = lib.rt_pixel_workspace_bytes(scene, len(qpx))
        d_ws = torch.empty(need, dtype=torch.uint8, device=dev)
        d_pix = torch.empty((len(qpx), 8), dtype=torch.float32, device=dev)
        d_smp = torch.empty((nq, 8), dtype=torch.float32, device=dev)
        d_ctr = torch.zeros(6, dtype=torch.int64, device=dev)

        def query():
            ok(lib.rt_pixel_query_async(scene, C.byref(cam), C.byref(p), d_qpx.data_ptr(), len(qpx), d_pix.data_ptr(),
                                        None, d_ws.data_ptr(), need, None, stream()), "rt_pixel_query_async")

        def q_rays():
            ok(lib.rt_camera_rays_async(scene, C.byref(cam), C.byref(p), d_qpx.data_ptr(), len(qpx), 0, spp,
                                        d_ws.data_ptr(), stream()), "rt_camera_rays_async")

        def q_paths():
            ok(lib.rt_path_rays_async(scene, d_ws.data_ptr(), nq, mb, flags, d_smp.data_ptr(), None, stream()),
               "rt_path_rays_async")

        t_q, t_qr, t_qp = timed(query, a.reps), timed(q_rays, a.reps), timed(q_paths, a.reps)
        t_q2, t_qp2 = timed(query, a.reps), timed(q_paths, a.reps)
        fold = t_q["ms_median"] - t_qr["ms_median"] - t_qp["ms_median"]
        ok(lib.rt_pixel_query_async(scene, C.byref(cam), C.byref(p), d_qpx.data_ptr(), len(qpx), d_pix.data_ptr(),
                                    d_smp.data_ptr(), d_ws.data_ptr(), need, d_ctr.data_ptr(), stream()), "query")
        torch.cuda.synchronize()
        # checks: the block's tile of the render, and the whole-frame rays against the 500-sample ones
        tile = R.RtParams.from_buffer_copy(p)
        tile.tile_x0, tile.tile_y0, tile.tile_w, tile.tile_h = x0, y0, b, b
        d_img = torch.zeros((p.height, p.width, 4), dtype=torch.float32, device=dev)
        d_dep = torch.zeros((p.height, p.width), dtype=torch.float32, device=dev)
        ok(lib.rt_render_image_async(scene, C.byref(cam), C.byref(tile), d_img.data_ptr(), d_dep.data_ptr(), None,
                                     stream()), "rt_render_image_async")
        torch.cuda.synchronize()
        pix = d_pix.view(torch.int32)
        same_rgba = bool(torch.equal(pix[:, :4].reshape(b, b, 4), d_img[y0:y0 + b, x0:x0 + b].view(torch.int32)))
        same_depth = bool(torch.equal(pix[:, 4].reshape(b, b), d_dep[y0:y0 + b, x0:x0 + b].view(torch.int32)))
        # the first 4096 pixels of the frame set, their 500-sample rays against the 16-sample call's
        d_r2 = torch.empty((4096 * spp, 8), dtype=torch.float32, device=dev)
        ok(lib.rt_camera_rays_async(scene, C.byref(cam), C.byref(p), d_px.data_ptr(), 4096, 0, spp, d_r2.data_ptr(),
                                    stream()), "rt_camera_rays_async")
        torch.cuda.synchronize()
        same_rays = bool(torch.equal(first, d_r2.view(torch.int32).reshape(4096, spp, 8)[:, :a.samples]))
        ctr = [int(v) for v in d_ctr.cpu().tolist()]
        res["pixel_query"] = {
            "block": [x0, y0, b, b], "pixels": len(qpx), "spp": spp, "paths": nq, "segments": ctr[0],
            "workspace_bytes": int(need),
            "rt_pixel_query_async": {**t_q, "again": t_q2},
            "parts_alone": {"rt_camera_rays_async": t_qr, "rt_path_rays_async": {**t_qp, "again": t_qp2}},
            "sum_of_rays_and_paths_alone_ms": round(t_qr["ms_median"] + t_qp["ms_median"], 4),
            "fold_by_difference_ms": round(fold, 4),
            "fold_share_of_query": round(fold / t_q["ms_median"], 4),
            "pixels_equal_render_tile": same_rgba and same_depth,
            "rays_equal_across_sample_ranges": same_rays}
    finally:
        torch.cuda.synchronize()
        lib.rt_dev_scene_free(scene)
    out = {"tool": "tools/pixels_bench.py", "scene": "C3: In-Next-Week 01, 10k moving spheres (seed 1234)",
           "objects": sc.n, "frame": [p.width, p.height], "table_spp": spp, "max_bounces": mb, "flags": flags, **res,
           "kernels": {name: R.pixels_kernel_info(i) for i, name in enumerate(R.PIXELS_KERNELS) if "IOW" not in name},
           "options": "defaults",
           "timing": f"HIP events around each call, {a.reps} timed launches after 3 warm-up launches; median, min, max"}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    if not (res["pixel_query"]["pixels_equal_render_tile"] and res["pixel_query"]["rays_equal_across_sample_ranges"]):
        raise SystemExit("pixel query and render disagree")


if __name__ == "__main__":
    main()
