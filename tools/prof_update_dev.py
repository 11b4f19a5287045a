"""rt_dev_scene_inw_update_device measured against rt_dev_scene_inw_update, one process,
warm-up first, the arms alternating call by call in an order that rotates, medians with [min, max]:

  host         rt_pack_inw + rt_dev_scene_inw_update with host pointers (nodes = NULL)
  dev_no_bins  rt_dev_scene_inw_update_device, RT_UPDATE_NO_BINS, records and boxes resident on the device
  dev_bins     rt_dev_scene_inw_update_device, RT_UPDATE_BINS
  fresh        no update: the frame of a fresh host-built scene, for scale

Per arm: the call's host time, its timing_ms, the time of the frame that follows (the scene's own frame:
C3 is 1920 x 1080, 500 spp, default options) and their sum; the frames' images must be equal.  The rule
for flags = 0: RT_UPDATE_BINS when its update + frame sum is the smaller one on C3 and the two sums do not lie
inside each other's [min, max]; otherwise RT_UPDATE_NO_BINS, the cheaper update.

python tools/prof_update_dev.py [--scene c3|large] [--reps 20] [--warmup 3] [--out profiles/update_dev_c3.json]
                                [--tree DIR]             (import rt_amd and its library from another checkout,
                                                          e.g. the parent commit's: only the arms it has)
                                [--width W --height H --spp S]   (a smaller frame, for a rehearsal)
                                [--embed KEY=FILE ...]   (other JSON results to keep beside these)"""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def mmm(v):
    """median [min, max] of a list, rounded"""
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def inside(a, b):
    """a's median + spread and b's lie inside each other's [min, max]"""
    return b["min"] <= a["median"] <= b["max"] and a["min"] <= b["median"] <= a["max"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="c3", choices=("c3", "large"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--out", default="")
    ap.add_argument("--width", type=int, default=0)
    ap.add_argument("--height", type=int, default=0)
    ap.add_argument("--spp", type=int, default=0)
    ap.add_argument("--embed", action="append", default=[])
    a = ap.parse_args()
    tree = os.path.abspath(a.tree)
    sys.path[:0] = [tree, os.path.join(tree, "raytracing-tests_amd")]
    import rt_amd as R
    import torch

    lib = R.load()
    if lib.rt_device_info(-1, None, 0, None) != 0:
        raise SystemExit("no gfx950 device: nothing is measured without one")
    over = {k: v for k, v in (("width", a.width), ("height", a.height), ("spp", a.spp)) if v}
    n_hint = 10_000 if a.scene == "c3" else 200_000
    sc = R.make_scene(R.PRESET_INW01_RANDOM, 1234, n_hint, **over)
    p = sc.params
    has_dev = hasattr(R, "update_inw_device")
    arms = ["host"] + (["dev_no_bins", "dev_bins"] if has_dev else []) + ["fresh"]
    dev = torch.device("cuda")
    img = torch.zeros((p.height, p.width, 4), dtype=torch.float32, device=dev)
    dep = torch.zeros((p.height, p.width), dtype=torch.float32, device=dev)
    ctr = torch.zeros(6, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def frame(s):
        ctr.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = lib.rt_render_image_async(s, C.byref(sc.camera), C.byref(p), img.data_ptr(), dep.data_ptr(), ctr.data_ptr(),
                                       stream)
        assert rc == 0, rc
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        return ms, hashlib.sha1(img.cpu().numpy().tobytes()).hexdigest()

    handles = {k: lib.rt_dev_scene_inw(R.fptr(sc.geom), sc.n, 1, R.fptr(sc.nodes), None, 0, p.spp, -1) for k in arms}
    assert all(handles.values())
    d_geom = torch.from_numpy(np.ascontiguousarray(sc.geom, np.float32)).to(dev)
    d_aabbs = torch.from_numpy(np.ascontiguousarray(sc.aabbs, np.float32)).to(dev)
    rows = {k: {"call_ms": [], "frame_ms": [], "sum_ms": [], "timing_ms": [[], [], [], []]} for k in arms}
    info, shas = {}, set()
    by_pos = [[] for _ in arms]  # the calls' times by their place in the round, whatever the arm
    tm = (C.c_double * 4)()
    try:
        for rep in range(a.warmup + a.reps):
            # the order rotates with the call, so nothing that depends on an arm's place in the round (what
            # ran before it, a periodic stall of the host) lands on the same arm every time
            for pos, name in enumerate(arms[rep % len(arms):] + arms[:rep % len(arms)]):
                s = handles[name]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if name == "host":
                    pk = R.pack(sc.desc, sc.n, sc.stage, build_lbvh=False)
                    rc = lib.rt_dev_scene_inw_update(s, R.fptr(pk["geom"]), sc.n, None, R.fptr(pk["aabbs"]), None, 0, tm)
                    assert rc == 0, rc
                    t = list(tm)
                elif name == "fresh":
                    t = [0.0] * 4
                else:
                    t = R.update_inw_device(s, d_geom, sc.n, d_aabbs,
                                            flags=R.RT_UPDATE_BINS if name == "dev_bins" else R.RT_UPDATE_NO_BINS,
                                            stream=stream)
                call = (time.perf_counter() - t0) * 1e3
                ms, sha = frame(s)
                shas.add(sha)
                if rep >= a.warmup:
                    r = rows[name]
                    r["call_ms"].append(call); r["frame_ms"].append(ms); r["sum_ms"].append(call + ms)
                    by_pos[pos].append(call)
                    for k in range(4):
                        r["timing_ms"][k].append(t[k])
        for name in arms:
            wi = (C.c_uint32 * 8)()
            lib.rt_debug_wide_info(handles[name], wi, None)
            info[name] = {"wide_info": list(wi), "time_bins": R.debug_path(handles[name])["time_bins"]}
    finally:
        for h in handles.values():
            lib.rt_dev_scene_free(h)
    res = {"scene": {"preset": "INW01_RANDOM", "seed": 1234, "objects": sc.n, "width": p.width, "height": p.height,
                     "spp": p.spp, "max_bounces": p.max_bounces},
           "tree": os.path.relpath(tree, ROOT), "reps": a.reps, "warmup": a.warmup, "images_equal": len(shas) == 1,
           "call_ms_by_place_in_round": [mmm(v) for v in by_pos],
           "arms": {k: {"call_ms": mmm(r["call_ms"]), "frame_ms": mmm(r["frame_ms"]), "sum_ms": mmm(r["sum_ms"]),
                        "timing_ms": [mmm(v) for v in r["timing_ms"]], **info[k]} for k, r in rows.items()}}
    if has_dev:
        A = res["arms"]
        res["device_to_device_saving_ms"] = round(A["host"]["call_ms"]["median"] - A["dev_no_bins"]["call_ms"]["median"], 4)
        nb, b = A["dev_no_bins"]["sum_ms"], A["dev_bins"]["sum_ms"]
        res["flags0_rule"] = {"sums_inside_each_other": inside(nb, b),
                              "choice": "RT_UPDATE_BINS" if b["median"] < nb["median"] and not inside(nb, b)
                              else "RT_UPDATE_NO_BINS"}
        if has_dev and hasattr(R, "update_kernel_info"):
            res["kernels"] = {name: R.update_kernel_info(i) for i, name in enumerate(R.UPDATE_KERNELS)}
    for e in a.embed:
        key, path = e.split("=", 1)
        res[key] = [json.loads(ln) for ln in open(path) if ln.strip().startswith("{")]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
