"""Times of the adaptive sample passes on packed tile lists and on a device group (rt_render_pass_slots_async,
rt_pass_select_tiles_async, rt_render_adaptive_multi_async) beside the single-device pair
(rt_render_pass_pixels_async, rt_pass_select_async) of the same build, at workload size.

  c3  the bench scene (In-Next-Week 01, 10k moving spheres, seed 1234, 1920x1080, 500 spp), batches of 16
  c2  the IOW-03 final scene (1200x800, 100 spp), batches of 10

Per scene, the two arms of each pair alternate launch by launch, --reps times after a warm-up (median [min, max];
a difference counts only where the two [min, max] ranges lie outside each other: `apart`):
  pass    a listed pass from count 0 over every slot of the one-device deal of the frame in 16x16 tiles
          (rt_tile_deal, row-major), beside a listed pass over every pixel in the rectangle's unit order (HIP
          events);
  select  rt_pass_select_tiles_async on that list's state beside rt_pass_select_async (HIP events);
  loop    the whole loop of a one-device group (rt_render_adaptive_multi_async rounds with image, depth and
          counts gathered every round, rt_group_adaptive_active between them) beside the single-device loop
          (pass + select + the read-back of n_active per round), at the median of the error image after the
          first round, tools/adaptive_bench.py's first tolerance (host clock around the loop, the device
          drained before and after: a group round waits on the host).
Exactness: the group loop's image, depth and counts against the single-device loop's, bit for bit.
Prints one JSON line per scene and writes it to --out-c3 / --out-c2.  Needs an MI355X.
    python tools/adaptive_tiles_bench.py [--scene c3|c2|both] [--reps 5] [--out-c3 ...] [--out-c2 ...]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "raytracing-tests_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import rt_amd as R  # noqa: E402

TILE = 16
SCENES = {"c3": dict(batch=16, iow=False), "c2": dict(batch=10, iow=True)}


def stream():
    return torch.cuda.current_stream().cuda_stream


def ok(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} -> {rc}")


def summary(ms):
    ms = sorted(ms)
    return {"ms_median": round(ms[len(ms) // 2], 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4), "n": len(ms)}


def pair(new, old):
    """Two summaries: the ratio of the medians, and whether the [min, max] ranges lie outside each other."""
    apart = new["ms_min"] > old["ms_max"] or new["ms_max"] < old["ms_min"]
    return {"new": new, "old": old, "new_over_old": round(new["ms_median"] / old["ms_median"], 4), "apart": apart}


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def host_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def alternate(new, old, reps, clock, pre=None):
    """new and old in turn, one warm-up each, then reps timed launches each; pre() before every launch."""
    ms = {"new": [], "old": []}
    for i in range(reps + 1):
        for k, fn in (("new", new), ("old", old)):
            if pre:
                pre()
            t = clock(fn)
            if i:
                ms[k].append(t)
    return pair(summary(ms["new"]), summary(ms["old"]))


def measure(lib, dev, name, reps):
    cfg = SCENES[name]
    if name == "c3":
        sc = R.make_scene(R.PRESET_INW01_RANDOM, 1234, 10_000, width=1920, height=1080, spp=500)
    else:
        sc = R.make_scene(R.PRESET_IOW03_FINAL, 20250131, 0)
    p, cam, batch = sc.params, sc.camera, cfg["batch"]
    W, H = int(p.width), int(p.height)
    npx = W * H
    tiles = np.asarray(R.tile_deal(W, H, TILE, 1), np.int32).reshape(-1, 2)
    n_tiles, n_slots = len(tiles), len(tiles) * TILE * TILE
    scene = R.dev_scene(sc, device=0)
    res = {"scene": name, "frame": [W, H], "spp": int(p.spp), "batch": batch, "tile_size": TILE, "tiles": n_tiles,
           "slots": n_slots, "slots_inside": npx, "reps": reps}
    try:
        z = lambda n, w, dt=torch.float32: torch.zeros((n, w), dtype=dt, device=dev)  # noqa: E731
        # the single-device buffers and the packed ones
        o = dict(state=z(npx, 8), aux=z(npx, 4, torch.int32), rgba=z(npx, 4), depth=z(npx, 1), err=z(npx, 1),
                 list=z(npx, 2, torch.int32), n=z(4, 1, torch.int32))
        t = dict(state=z(n_slots, 8), aux=z(n_slots, 4, torch.int32), rgba=z(n_slots, 4), depth=z(n_slots, 1),
                 err=z(n_slots, 1), list=z(n_slots, 1, torch.int32), n=z(4, 1, torch.int32),
                 tiles=torch.from_numpy(tiles.copy()).to(dev))

        def old_select(tol, m=2):
            ok(R.pass_select(scene, p, o["state"], o["aux"], tol, m, o["list"], o["n"], o["err"], stream()),
               "rt_pass_select_async")

        def new_select(tol, m=2):
            ok(R.pass_select_tiles(scene, p, t["tiles"], n_tiles, TILE, t["state"], t["aux"], tol, m, t["list"], t["n"],
                                   t["err"], stream()), "rt_pass_select_tiles_async")

        def old_pass(n):
            ok(R.pass_pixels(scene, cam, p, o["list"], n, batch, o["state"], o["aux"], o["rgba"], o["depth"], None,
                             stream()), "rt_render_pass_pixels_async")

        def new_pass(n):
            ok(R.pass_slots(scene, cam, p, t["tiles"], n_tiles, TILE, t["list"], n, batch, t["state"], t["aux"], t["rgba"],
                            t["depth"], None, stream()), "rt_render_pass_slots_async")

        old_select(-1.0, 0)
        new_select(-1.0, 0)
        torch.cuda.synchronize()
        assert int(o["n"][0].item()) == npx and int(t["n"][0].item()) == npx

        def zero_aux():
            o["aux"].zero_()
            t["aux"].zero_()

        res["pass"] = alternate(lambda: new_pass(npx), lambda: old_pass(npx), reps, event_ms, pre=zero_aux)
        # the selects on the state that pass left
        res["select"] = alternate(lambda: new_select(0.01), lambda: old_select(0.01), reps, event_ms)
        first_err = o["err"].cpu().numpy().reshape(-1)
        tol = float(np.median(first_err[np.isfinite(first_err)]))
        res["tol"] = tol

        # ---- the loops
        def old_loop():
            o["aux"].zero_()
            old_select(-1.0, 0)
            n, rounds = int(o["n"][0].item()), 0
            while n > 0:
                old_pass(n)
                old_select(tol)
                n = int(o["n"][0].item())  # synchronises: the loop's read-back
                rounds += 1
            return rounds

        grp = lib.rt_group_create((C.c_int * 1)(0), 1)
        if not grp:
            raise RuntimeError("rt_group_create failed")
        scenes = (C.c_void_p * 1)(scene)
        g = dict(rgba=z(npx, 4), depth=z(npx, 1), count=z(npx, 1, torch.int32))
        try:
            def new_loop():
                n, rounds = 1, 0
                while n > 0:
                    ok(R.render_adaptive_multi_round(grp, scenes, cam, p, TILE, rounds == 0, batch, tol, 2, g["rgba"],
                                                     g["depth"], g["count"], None, stream()),
                       "rt_render_adaptive_multi_async")
                    n = R.group_adaptive_active(grp)
                    rounds += 1
                return rounds

            rounds = (new_loop(), old_loop())
            torch.cuda.synchronize()
            depth_same = cfg["iow"] or torch.equal(g["depth"].view(torch.int32), o["depth"].view(torch.int32))
            res["exactness"] = {"rounds": list(rounds), "rounds_equal": rounds[0] == rounds[1],
                                "rgba_equal": bool(torch.equal(g["rgba"].view(torch.int32), o["rgba"].view(torch.int32))),
                                "depth_equal": bool(depth_same),
                                "counts_equal": bool(torch.equal(g["count"].view(-1), o["aux"][:, 3]))}
            samples = int(o["aux"][:, 3].to(torch.int64).sum().item())
            res["loop"] = {**alternate(new_loop, old_loop, reps, host_ms), "rounds": rounds[1], "samples": samples,
                           "samples_over_full": round(samples / (npx * int(p.spp)), 4)}
        finally:
            torch.cuda.synchronize()
            lib.rt_group_free(grp)
    finally:
        torch.cuda.synchronize()
        lib.rt_dev_scene_free(scene)
    old = (10, 11) if cfg["iow"] else (8, 9)
    new = (26, 27) if cfg["iow"] else (24, 25)
    res["kernels"] = {**{R.ADAPTIVE_KERNELS[i]: R.pass_kernel_info(i) for i in old + (12, 14)},
                      **{R.ADAPTIVE_TILE_KERNELS[i]: R.pass_kernel_info(i) for i in new + (28, 30)}}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", choices=("c3", "c2", "both"), default="both")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out-c3", default=None)
    ap.add_argument("--out-c2", default=None)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    lib = R.load()
    if lib.rt_device_info(0, None, 0, None) != 0:
        raise RuntimeError("no gfx950 device: the times are measured on the GPU or not at all")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    bad = False
    for name, path in (("c3", a.out_c3), ("c2", a.out_c2)):
        if a.scene not in (name, "both"):
            continue
        out = {"tool": "tools/adaptive_tiles_bench.py", **measure(lib, dev, name, a.reps)}
        out["timing"] = "the two arms alternate; one warm-up launch each, then the timed ones; median, min, max"
        print(json.dumps(out), flush=True)
        if path:
            with open(path, "w") as f:
                f.write(json.dumps(out, indent=1) + "\n")
        e = out["exactness"]
        bad |= not (e["rounds_equal"] and e["rgba_equal"] and e["depth_equal"] and e["counts_equal"])
    if bad:
        raise SystemExit("the group loop and the single-device loop disagree")


if __name__ == "__main__":
    main()
