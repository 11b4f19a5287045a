"""Times of the progressive sample passes over packed tile lists and on a device group
(rt_render_pass_tiles_async, rt_render_pass_multi_async) beside the rectangle passes (rt_render_pass_async),
at workload size, and the rectangle passes of this library beside those of another build of it.

  c3  the bench scene (In-Next-Week 01, 10k moving spheres, seed 1234, 1920x1080, 500 spp): the frame as
      32 passes of 16 samples (the last one clipped), the cuts tools/passes_bench.py uses.
  c2  the IOW-03 final scene (1200x800, 100 spp): the frame as 10 passes of 10 samples.

Per scene, a frame of passes is timed (HIP events around the whole frame, warm-up frames first, then --reps
timed ones; median [min, max]):
  rect        rt_render_pass_async on the whole frame;
  tiles       rt_render_pass_tiles_async on every 16x16 tile of the frame in the hashed order of the
              8-device deal (rt_tile_deal), one device; rect and tiles alternate frame by frame;
  share       the same on each share of the 8-device deal, once each, and the slowest one --reps times;
  group       a one-device group: rt_render_pass_multi_async with the image gathered by every pass, with the
              image gathered by the last pass alone (c3 only), and one rt_render_multi_async frame.
With --parent-lib the rect frame is also timed with that library (the parent commit's build) in processes
of its own, alternating with this library's: other, this, other, this.  The first "this" is the rect arm
above (in the process that also times tiles, shares and group, frame by frame beside the tiles arm), the
second a process that times rect alone.  `rect_vs_parent.inside` says whether both medians of this library
lie inside the other's [min, max]; the tool exits non-zero when they do not.

Every child is a fresh process (one process has the GPU open at a time); a child that fails ends the run.
Prints one JSON line per scene and writes it to --out-c3 / --out-c2.  Needs an MI355X.
    python tools/pass_tiles_bench.py [--scene c3|c2|both] [--parent-lib PATH] [--out-c3 ...] [--out-c2 ...]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "raytracing-tests_amd")]

NEW = ("rt_render_pass_tiles_async", "rt_render_pass_multi_async", "rt_render_passes_inw_multi")
# (c2: a frame of passes takes 17 s, so fewer frames, and the exchange's cost is measured on c3 alone)
SCENES = {"c3": dict(ns=16, warm=3, reps=20, counters=(0, 3, 4, 5), exchange=True),
          "c2": dict(ns=10, warm=1, reps=3, counters=(0, 4, 5), exchange=False)}
TILE = 16
DEAL = 8


def summary(ms):
    ms = sorted(ms)
    return {"ms_median": round(ms[len(ms) // 2], 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4), "n": len(ms)}


def ok(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} -> {rc}")


# ----------------------------------------------------------------------------------------- a child: one arm
def child(a):
    import numpy as np
    import torch

    import rt_amd as R

    if a.lib:  # another build of the library: it may lack the new entry points
        probe = C.CDLL(a.lib)
        for name in NEW:
            if not hasattr(probe, name):
                R.capi.SIGNATURES.pop(name, None)
    lib = R.load(a.lib) if a.lib else R.load()
    if lib.rt_device_info(0, None, 0, None) != 0:
        raise RuntimeError("no gfx950 device: the times are measured on the GPU or not at all")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    cfg = SCENES[a.scene]
    reps, warm, ns = a.reps or cfg["reps"], cfg["warm"], cfg["ns"]
    if a.scene == "c3":
        sc = R.make_scene(R.PRESET_INW01_RANDOM, 1234, 10_000, width=1920, height=1080, spp=500)
    else:
        sc = R.make_scene(R.PRESET_IOW03_FINAL, 20250131, 0)
    p, cam = sc.params, sc.camera
    W, H, spp = int(p.width), int(p.height), int(p.spp)
    starts = list(range(0, spp, ns))
    stream = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
    scene = R.dev_scene(sc, device=0)

    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def note(what):
        print(f"[pass_tiles_bench]   {what}", file=sys.stderr, flush=True)

    def interleaved(fns):
        """Every arm `warm` frames, then the arms in turn, frame by frame, `reps` times."""
        for fn in fns.values():
            for _ in range(warm):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in fns}
        for i in range(reps):
            for k, fn in fns.items():
                ms[k].append(once(fn))
            note(f"{' / '.join(fns)}: frame {i + 1} of {reps}")
        return {k: summary(v) for k, v in ms.items()}

    n = W * H
    state = torch.zeros((n, 8), dtype=torch.float32, device=dev)
    rgba = torch.zeros((n, 4), dtype=torch.float32, device=dev)
    depth = torch.zeros(n, dtype=torch.float32, device=dev)
    ctr = torch.zeros(6, dtype=torch.int64, device=dev)

    def rect_frame(counters=None):
        for s0 in starts:
            ok(lib.rt_render_pass_async(scene, C.byref(cam), C.byref(p), s0, ns, state.data_ptr(), rgba.data_ptr(),
                                        depth.data_ptr(), counters, stream()), "rt_render_pass_async")

    res = {"scene": a.scene, "lib": "other build" if a.lib else "this", "passes": len(starts), "samples_per_pass": ns,
           "warm": warm, "reps": reps}
    try:
        if a.child == "rect":
            res["rect"] = interleaved({"rect": rect_frame})["rect"]
            return res
        # ---- the whole frame as one tile list, hashed order
        order = np.asarray(R.tile_deal(W, H, TILE, DEAL), np.int32).reshape(-1, 2)
        area = TILE * TILE

        class List:
            def __init__(self, tiles):
                self.n = len(tiles)
                self.d_tiles = torch.from_numpy(np.ascontiguousarray(tiles)).to(dev)
                self.state = torch.zeros((self.n * area, 8), dtype=torch.float32, device=dev)
                self.rgba = torch.zeros((self.n * area, 4), dtype=torch.float32, device=dev)
                self.depth = torch.zeros(self.n * area, dtype=torch.float32, device=dev)

            def frame(self, counters=None):
                for s0 in starts:
                    ok(lib.rt_render_pass_tiles_async(scene, C.byref(cam), C.byref(p), self.d_tiles.data_ptr(), self.n,
                                                      TILE, s0, ns, self.state.data_ptr(), self.rgba.data_ptr(),
                                                      self.depth.data_ptr(), counters, stream()),
                       "rt_render_pass_tiles_async")

        full = List(order)
        t = interleaved({"rect": rect_frame, "tiles": full.frame})
        res.update(t)
        res["tiles_over_rect"] = round(t["tiles"]["ms_median"] / t["rect"]["ms_median"], 4)
        # exactness: the last pass against rt_render_tiles_async of the same list, and the counters against the rect passes'
        ctr.zero_()
        rect_frame(ctr.data_ptr())
        torch.cuda.synchronize()
        rect_ctr = [int(v) for v in ctr.cpu().tolist()]
        ctr.zero_()
        full.frame(ctr.data_ptr())
        want = torch.zeros_like(full.rgba)
        want_depth = torch.zeros_like(full.depth)
        ok(lib.rt_render_tiles_async(scene, C.byref(cam), C.byref(p), full.d_tiles.data_ptr(), full.n, TILE,
                                     want.data_ptr(), want_depth.data_ptr(), None, stream()), "rt_render_tiles_async")
        torch.cuda.synchronize()
        tile_ctr = [int(v) for v in ctr.cpu().tolist()]
        res["exactness"] = {"rgba_equal_tile_render": bool(torch.equal(full.rgba.view(torch.int32), want.view(torch.int32))),
                            "depth_equal_tile_render": bool(torch.equal(full.depth.view(torch.int32),
                                                                        want_depth.view(torch.int32))),
                            "counters_equal_rect_passes": all(tile_ctr[k] == rect_ctr[k] for k in cfg["counters"]),
                            "segments": tile_ctr[0]}
        final = rgba.clone()
        note(f"exactness {res['exactness']}")
        del full, want, want_depth
        # ---- the shares of the 8-device deal: each once, the slowest `reps` times
        shares = [List(order[r::DEAL]) for r in range(DEAL)]
        shares[0].frame()
        torch.cuda.synchronize()
        each = [round(once(s.frame), 4) for s in shares]
        slow = max(range(DEAL), key=lambda r: each[r])
        res["shares"] = {"n_dev": DEAL, "tiles": [s.n for s in shares], "each_ms": each, "slowest": slow,
                         "slowest_frame": summary([once(shares[slow].frame) for _ in range(reps)])}
        res["shares"]["slowest_over_rect"] = round(res["shares"]["slowest_frame"]["ms_median"] / t["rect"]["ms_median"], 4)
        res["shares"]["slowest_over_tiles_eighth"] = round(res["shares"]["slowest_frame"]["ms_median"] * DEAL /
                                                           t["tiles"]["ms_median"], 4)
        del shares
        note("shares done")
        # ---- a one-device group
        grp = lib.rt_group_create((C.c_int * 1)(0), 1)
        if not grp:
            raise RuntimeError("rt_group_create failed")
        scenes = (C.c_void_p * 1)(scene)
        try:
            def group_frame(every):
                for i, s0 in enumerate(starts):
                    img = every or i == len(starts) - 1
                    ok(lib.rt_render_pass_multi_async(grp, scenes, C.byref(cam), C.byref(p), TILE, s0, ns,
                                                      rgba.data_ptr() if img else None, depth.data_ptr() if img else None,
                                                      None, stream()), "rt_render_pass_multi_async")

            def multi_frame():
                ok(lib.rt_render_multi_async(grp, scenes, C.byref(cam), C.byref(p), TILE, rgba.data_ptr(),
                                             depth.data_ptr(), None, stream()), "rt_render_multi_async")

            arms = {"passes_image_every_pass": lambda: group_frame(True), "multi_frame": multi_frame}
            if cfg["exchange"]:
                arms["passes_image_last_pass"] = lambda: group_frame(False)
            g = interleaved(arms)
            group_frame(True)
            torch.cuda.synchronize()
            g["rgba_equal_rect_passes"] = bool(torch.equal(rgba.view(torch.int32), final.view(torch.int32)))
            if cfg["exchange"]:
                g["exchange_ms_per_pass"] = round((g["passes_image_every_pass"]["ms_median"] -
                                                   g["passes_image_last_pass"]["ms_median"]) / max(1, len(starts) - 1), 4)
            g["passes_over_multi_frame"] = round(g["passes_image_every_pass"]["ms_median"] /
                                                 g["multi_frame"]["ms_median"], 4)
            g["devices"] = 1
            res["group"] = g
        finally:
            torch.cuda.synchronize()
            lib.rt_group_free(grp)
        res["kernels"] = {name: R.pass_kernel_info(which) for which, name in R.PASS_TILE_KERNELS.items()}
        return res
    finally:
        torch.cuda.synchronize()
        lib.rt_dev_scene_free(scene)


# ----------------------------------------------------------------------------------------- the driver
def run_child(a, scene, mode, lib):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--scene", scene]
    if lib:
        cmd += ["--lib", lib]
    if a.reps:
        cmd += ["--reps", str(a.reps)]
    print(f"[pass_tiles_bench] {scene} {mode} {lib or 'this library'}", file=sys.stderr, flush=True)
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.child_timeout)  # stderr: progress, passed on
    if r.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)} -> {r.returncode}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", choices=("c3", "c2", "both"), default="both")
    ap.add_argument("--reps", type=int, default=0, help="timed frames per arm (default: 20 on c3, 3 on c2)")
    ap.add_argument("--parent-lib", default=None, help="another build of librt_hip.so to time the rect passes with")
    ap.add_argument("--out-c3", default=None)
    ap.add_argument("--out-c2", default=None)
    ap.add_argument("--child-timeout", type=int, default=900)
    ap.add_argument("--child", choices=("rect", "full"), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--lib", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child(a)), flush=True)
        return
    bad = False
    for scene, path in (("c3", a.out_c3), ("c2", a.out_c2)):
        if a.scene not in (scene, "both"):
            continue
        out = {"tool": "tools/pass_tiles_bench.py", "tile_size": TILE}
        if a.parent_lib:
            other = [run_child(a, scene, "rect", a.parent_lib)]
            full = run_child(a, scene, "full", None)
            other.append(run_child(a, scene, "rect", a.parent_lib))
            again = run_child(a, scene, "rect", None)
            lo = min(o["rect"]["ms_min"] for o in other)
            hi = max(o["rect"]["ms_max"] for o in other)
            this = [full["rect"], again["rect"]]
            med = sorted(t["ms_median"] for t in this)
            out["rect_vs_parent"] = {"order": "other, this, other, this (a process each)",
                                     "other": [o["rect"] for o in other], "this": this,
                                     "other_min_max": [lo, hi], "this_medians": med,
                                     "inside": all(lo <= m <= hi for m in med)}
        else:
            full = run_child(a, scene, "full", None)
        out.update(full)
        out["timing"] = "HIP events around a frame of passes; warm-up frames, then timed ones; median, min, max"
        print(json.dumps(out), flush=True)
        if path:
            with open(path, "w") as f:
                f.write(json.dumps(out, indent=1) + "\n")
        e, g = out["exactness"], out["group"]
        bad |= not (e["rgba_equal_tile_render"] and e["counters_equal_rect_passes"] and g["rgba_equal_rect_passes"])
        bad |= not out.get("rect_vs_parent", {"inside": True})["inside"]
    if bad:
        raise SystemExit("the tile-list passes and the renders disagree, or the rectangle passes left the other "
                         "library's [min, max]")


if __name__ == "__main__":
    main()
