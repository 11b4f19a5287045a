"""Times of the progressive sample passes (rt_render_pass_async; INW: k_pass_rays, k_inw_paths and
k_pass_fold per chunk of samples; IOW-03: k_iow_pass) beside the composition that gives the same samples without them (rt_camera_rays_async plus the path queries on the
frame's pixels in 8x8-block order), and their exactness at workload size.

  c3  the bench scene (In-Next-Week 01, 10k moving spheres, seed 1234, 1920x1080, 500 spp, 50 bounces):
      passes of --samples-c3 samples (16), the first (s0 = 0) and a middle one (s0 = 240), each timed
      alternating with rt_camera_rays_async + rt_path_rays_async for the same samples; all 500 samples as
      32 passes (the last one clipped), whose last image must equal rt_render_image_async's byte for
      byte; and, as context, the frame's own time and k_inw's (rt_options.inw_order = -1), scaled to 16
      samples.
  c2  the IOW-03 final scene (1200x800, 100 spp): passes of 10 samples, the first and a middle one
      (s0 = 50, from the state the five passes before it left, restored before every launch), beside
      rt_camera_rays_async + rt_path_iow_rays_async with chain = 10; all 100 samples as 10 passes, whose
      last image must equal rt_render_image_async's; and the frame's own time scaled to 10 samples.

Every time: HIP events around each call, 3 warm-up launches, then --reps timed ones; median [min, max].
A pass must not be slower than the composition by more than the spread of the alternating runs
(`verdict`).  Prints one JSON line per scene (and writes it to --out-c3 / --out-c2).  Needs an MI355X.
    python tools/passes_bench.py [--scene c3|c2|both] [--out-c3 profiles/passes_c3.json] [--out-c2 ...]
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


def block_pixels(w, h):
    """Every pixel of the w x h frame (multiples of 8) as (x, y) int32 pairs, 8x8 blocks row-major, each
    block row-major: the order the passes' units map to pixels."""
    ys, xs = np.meshgrid(np.arange(h, dtype=np.int32), np.arange(w, dtype=np.int32), indexing="ij")
    blk = lambda a: a.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3).reshape(-1)  # noqa: E731
    return np.stack([blk(xs), blk(ys)], axis=1)


def timed(fn, reps, warm=3, pre=None):
    """fn() enqueued on the current stream: {ms_median, ms_min, ms_max} over reps launches after warm;
    pre() runs before each launch, outside the events."""
    ev = []
    for i in range(warm + reps):
        if pre:
            pre()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        if i >= warm:
            ev.append((a, b))
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return {"ms_median": round(ms[len(ms) // 2], 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4)}


def ok(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} -> {rc}")


def alternate(f_pass, f_comp, reps, pre=None):
    """The pass and the composition timed in turn, twice each; the spread of the alternating runs is the
    larger of the two differences between a measurement's medians."""
    p1, c1 = timed(f_pass, reps, pre=pre), timed(f_comp, reps)
    p2, c2 = timed(f_pass, reps, pre=pre), timed(f_comp, reps)
    spread = max(abs(p1["ms_median"] - p2["ms_median"]), abs(c1["ms_median"] - c2["ms_median"]))
    pm, cm = min(p1["ms_median"], p2["ms_median"]), min(c1["ms_median"], c2["ms_median"])
    return {"pass": {**p1, "again": p2}, "composition": {**c1, "again": c2}, "spread_ms": round(spread, 4),
            "pass_over_composition": round(pm / cm, 4),
            "verdict": "pass not slower" if pm <= cm + spread else "PASS SLOWER"}


class Frame:
    """The device buffers of one frame's passes and renders."""

    def __init__(self, lib, scene, sc, dev):
        self.lib, self.scene, self.sc = lib, scene, sc
        p = sc.params
        n = p.width * p.height
        self.state = torch.zeros((n, 8), dtype=torch.float32, device=dev)
        self.rgba = torch.zeros((n, 4), dtype=torch.float32, device=dev)
        self.depth = torch.zeros(n, dtype=torch.float32, device=dev)
        self.ctr = torch.zeros(6, dtype=torch.int64, device=dev)

    def run(self, s0, ns, counters=False):
        sc = self.sc
        ok(self.lib.rt_render_pass_async(self.scene, C.byref(sc.camera), C.byref(sc.params), s0, ns,
                                         self.state.data_ptr(), self.rgba.data_ptr(), self.depth.data_ptr(),
                                         self.ctr.data_ptr() if counters else None,
                                         torch.cuda.current_stream().cuda_stream), "rt_render_pass_async")


def render(lib, scene, sc, dev, reps=0):
    """rt_render_image_async of the frame: (rgba, depth, counters, timing or None)."""
    p = sc.params
    n = p.width * p.height
    rgba = torch.zeros((n, 4), dtype=torch.float32, device=dev)
    depth = torch.zeros(n, dtype=torch.float32, device=dev)
    ctr = torch.zeros(6, dtype=torch.int64, device=dev)

    def go(c=None):
        ok(lib.rt_render_image_async(scene, C.byref(sc.camera), C.byref(p), rgba.data_ptr(), depth.data_ptr(), c,
                                     torch.cuda.current_stream().cuda_stream), "rt_render_image_async")

    go(ctr.data_ptr())
    torch.cuda.synchronize()
    t = timed(go, reps, warm=1) if reps else None
    return rgba, depth, [int(v) for v in ctr.cpu().tolist()], t


def exactness(fr, want, spp, ns, slots):
    """All spp samples as passes of ns (the last one clipped): the last image, depth and the counters
    against the render's; and the time of the whole sequence."""
    rgba, depth, ctr, _ = want
    starts = list(range(0, spp, ns))

    def frame(counters=False):
        for s0 in starts:
            fr.run(s0, ns, counters)

    fr.ctr.zero_()
    frame(True)
    torch.cuda.synchronize()
    got = [int(v) for v in fr.ctr.cpu().tolist()]
    res = {"passes": len(starts), "samples_per_pass": ns, "last_pass_samples": spp - starts[-1],
           "rgba_equal_render": bool(torch.equal(fr.rgba.view(torch.int32), rgba.view(torch.int32))),
           "depth_equal_render": bool(torch.equal(fr.depth.view(torch.int32), depth.view(torch.int32))),
           "counters_equal_render": all(got[k] == ctr[k] for k in slots), "segments": got[0]}
    res["all_passes"] = timed(frame, 3, warm=1)
    return res


def scaled(t, num, den):
    return round(t["ms_median"] * num / den, 4)


def bench_c3(lib, dev, a):
    sc = R.make_scene(R.PRESET_INW01_RANDOM, 1234, 10_000, width=1920, height=1080, spp=500)
    p, cam = sc.params, sc.camera
    spp, mb, ns = int(p.spp), int(p.max_bounces), a.samples_c3
    d = np.array(list(cam.dir), np.float32)
    flags = R.RT_TRACE_INVERT if np.float32(np.float32(d[0] + d[1]) + d[2]) > 0 else 0
    stream = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
    scene = R.dev_scene(sc, device=0)
    res = {}
    try:
        fr = Frame(lib, scene, sc, dev)
        px = block_pixels(p.width // 8 * 8, p.height // 8 * 8)
        d_px = torch.from_numpy(px.copy()).to(dev)
        n = len(px) * ns
        d_rays = torch.empty((n, 8), dtype=torch.float32, device=dev)
        d_out = torch.empty_like(d_rays)

        def comp(s0):
            ok(lib.rt_camera_rays_async(scene, C.byref(cam), C.byref(p), d_px.data_ptr(), len(px), s0, ns,
                                        d_rays.data_ptr(), stream()), "rt_camera_rays_async")
            ok(lib.rt_path_rays_async(scene, d_rays.data_ptr(), n, mb, flags, d_out.data_ptr(), None, stream()),
               "rt_path_rays_async")

        mid = 240
        res["first_pass"] = {"s0": 0, "ns": ns, **alternate(lambda: fr.run(0, ns), lambda: comp(0), a.reps)}
        res["middle_pass"] = {"s0": mid, "ns": ns, **alternate(lambda: fr.run(mid, ns), lambda: comp(mid), a.reps)}
        # the first form of the INW entry point (k_inw_pass: a lane owned a pixel for the whole pass),
        # as this tool measured it before it was replaced
        res["fused_kernel_before"] = {"first_pass_ms": [20.573, 21.0566], "middle_pass_ms": [20.3644, 20.148],
                                      "composition_ms_then": [9.5596, 9.664, 10.4373, 10.3192],
                                      "all_500_samples_as_32_passes_ms": 622.6874}
        del d_rays, d_out
        want = render(lib, scene, sc, dev, reps=5)
        res["exactness"] = exactness(fr, want, spp, ns, (0, 3, 4, 5))
        res["context"] = {"frame": want[3], "frame_share_of_a_pass_ms": scaled(want[3], ns, spp),
                          "all_passes_over_frame": round(res["exactness"]["all_passes"]["ms_median"] /
                                                         want[3]["ms_median"], 3)}
    finally:
        torch.cuda.synchronize()
        lib.rt_dev_scene_free(scene)
    with R.options(inw_order=-1):  # the per-pixel sequential kernel k_inw
        scene = R.dev_scene(sc, device=0)
    try:
        seq = render(lib, scene, sc, dev, reps=3)
        res["context"]["k_inw_frame"] = seq[3]
        res["context"]["k_inw_share_of_a_pass_ms"] = scaled(seq[3], ns, spp)
        res["context"]["k_inw_frame_equal"] = bool(torch.equal(seq[0].view(torch.int32), want[0].view(torch.int32)))
    finally:
        torch.cuda.synchronize()
        lib.rt_dev_scene_free(scene)
    return {"tool": "tools/passes_bench.py", "scene": "C3: In-Next-Week 01, 10k moving spheres (seed 1234)",
            "objects": sc.n, "frame": [p.width, p.height], "spp": spp, "max_bounces": mb, **res,
            "kernels": {R.PASS_KERNELS[i]: R.pass_kernel_info(i) for i in (0, 1)},
            "path_kernel": R.paths_kernel_info(False, True)}


def bench_c2(lib, dev, a):
    sc = R.make_scene(R.PRESET_IOW03_FINAL, 20250131, 0)
    p, cam = sc.params, sc.camera
    spp, mb, ns = int(p.spp), int(p.max_bounces), a.samples_c2
    stream = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
    scene = R.dev_scene(sc, device=0)
    res = {}
    try:
        fr = Frame(lib, scene, sc, dev)
        px = block_pixels(p.width // 8 * 8, p.height // 8 * 8)
        d_px = torch.from_numpy(px.copy()).to(dev)
        n = len(px) * ns
        d_rays = torch.empty((n, 12), dtype=torch.float32, device=dev)
        d_out = torch.empty_like(d_rays)

        def comp(s0):
            ok(lib.rt_camera_rays_async(scene, C.byref(cam), C.byref(p), d_px.data_ptr(), len(px), s0, ns,
                                        d_rays.data_ptr(), stream()), "rt_camera_rays_async")
            ok(lib.rt_path_iow_rays_async(scene, d_rays.data_ptr(), n, ns, mb, 0, d_out.data_ptr(), None, stream()),
               "rt_path_iow_rays_async")

        res["first_pass"] = {"s0": 0, "ns": ns, **alternate(lambda: fr.run(0, ns), lambda: comp(0), a.reps)}
        mid = (spp // ns // 2) * ns
        for s0 in range(0, mid, ns):
            fr.run(s0, ns)
        torch.cuda.synchronize()
        saved = fr.state.clone()
        res["middle_pass"] = {"s0": mid, "ns": ns,
                              "note": "the composition starts its chains from ri = 0, the pass from the pixels' states",
                              **alternate(lambda: fr.run(mid, ns), lambda: comp(mid), a.reps,
                                          pre=lambda: fr.state.copy_(saved))}
        del d_rays, d_out
        want = render(lib, scene, sc, dev, reps=3)
        want = (want[0], torch.zeros_like(want[1]), want[2], want[3])  # a pass writes the depth 0
        res["exactness"] = exactness(fr, want, spp, ns, (0, 4, 5))
        res["context"] = {"frame": want[3], "frame_share_of_a_pass_ms": scaled(want[3], ns, spp),
                          "all_passes_over_frame": round(res["exactness"]["all_passes"]["ms_median"] /
                                                         want[3]["ms_median"], 3)}
    finally:
        torch.cuda.synchronize()
        lib.rt_dev_scene_free(scene)
    return {"tool": "tools/passes_bench.py", "scene": "C2: In-One-Weekend 03 final scene (seed 20250131)",
            "objects": sc.n, "frame": [p.width, p.height], "spp": spp, "max_bounces": mb, **res,
            "kernels": {R.PASS_KERNELS[i]: R.pass_kernel_info(i) for i in (2, 3)},
            "path_kernel": R.path_iow_kernel_info(True)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", choices=("c3", "c2", "both"), default="both")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--samples-c3", type=int, default=16)
    ap.add_argument("--samples-c2", type=int, default=10)
    ap.add_argument("--out-c3", default=None)
    ap.add_argument("--out-c2", default=None)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    lib = R.load()
    if lib.rt_device_info(0, None, 0, None) != 0:
        raise RuntimeError("no gfx950 device: the times are measured on the GPU or not at all")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    bad = False
    for name, fn, path in (("c3", bench_c3, a.out_c3), ("c2", bench_c2, a.out_c2)):
        if a.scene not in (name, "both"):
            continue
        out = fn(lib, dev, a)
        out["options"] = "defaults"
        out["timing"] = f"HIP events around each call, {a.reps} timed launches after 3 warm-up launches; median, min, max"
        print(json.dumps(out), flush=True)
        if path:
            with open(path, "w") as f:
                f.write(json.dumps(out, indent=1) + "\n")
        e = out["exactness"]
        bad |= not (e["rgba_equal_render"] and e["depth_equal_render"] and e["counters_equal_render"])
    if bad:
        raise SystemExit("the last pass and the render disagree")


if __name__ == "__main__":
    main()
