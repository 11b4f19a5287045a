"""rt_dev_scene_iow03_update measured, one process, warm-up first, the variants
alternating, medians with [min, max]:

  update_vs_recreate  the C2 scene (IOW-03 final scene, 1200 x 800, 100 spp, default options): an edit
                      (every object moves) and its first frame by (a) rt_dev_scene_free +
                      rt_dev_scene_iow03, (b) the update with the host build, (c) with the device build
  builder             timing_ms[1] (boxes and culling BVH) of the host and the device build at several
                      object counts (C2's spheres tiled), and the flags = 0 rule they give: the device
                      build from the smallest measured n at which its median is below the host build's
                      by more than the host build's own spread (max - min)
  tree_quality        the C2 frame after a host-built and after a device-built update of the same records:
                      frame time, wide nodes, the LDS-staged instances, counters [1] and [2], images equal

python tools/prof_update_iow.py [--reps 5] [--builder-reps 15] [--out profiles/update_iow.json]
                                [--width W --height H --spp S]   (a smaller frame, for a rehearsal)
                                [--embed KEY=FILE ...]           (other JSON results to keep beside these)"""
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
sys.path[:0] = [ROOT, os.path.join(ROOT, "raytracing-tests_amd")]
import rt_amd as R  # noqa: E402

HOST, DEVICE = R.RT_UPDATE_HOST_BUILD, R.RT_UPDATE_DEVICE_BUILD


def mmm(v):
    """median [min, max] of a list, rounded"""
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def moved(rec, k):
    """the records with every object moved (edit number k: the offsets alternate, so edits never repeat
    the state before them)"""
    out = rec.copy()
    i = np.arange(len(rec))
    for a in range(3):
        out[:, a] += (0.02 * (k % 2 + 1) * ((i + a) % 3 - 1)).astype(np.float32)
    return np.ascontiguousarray(out)


class Frames:
    """device buffers of one frame size and a blocking render into them"""

    def __init__(self, sc):
        import torch
        self.torch = torch
        self.sc = sc
        p = sc.params
        dev = torch.device("cuda")
        self.img = torch.zeros((p.height, p.width, 4), dtype=torch.float32, device=dev)
        self.ctr = torch.zeros(6, dtype=torch.int64, device=dev)

    def render(self, s):
        """-> (host ms to the end of the frame, counters, sha1 of the image)"""
        torch, sc = self.torch, self.sc
        self.ctr.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = R.load().rt_render_image_async(s, C.byref(sc.camera), C.byref(sc.params), self.img.data_ptr(), None,
                                            self.ctr.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        return ms, [int(x) for x in self.ctr.cpu().numpy()], hashlib.sha1(self.img.cpu().numpy().tobytes()).hexdigest()


def update_vs_recreate(sc, reps):
    lib = R.load()
    fr = Frames(sc)
    spp = sc.params.spp
    handles = {"recreate": lib.rt_dev_scene_iow03(R.fptr(sc.types), R.fptr(sc.records), sc.n, spp, -1),
               "update_host": lib.rt_dev_scene_iow03(R.fptr(sc.types), R.fptr(sc.records), sc.n, spp, -1),
               "update_device": lib.rt_dev_scene_iow03(R.fptr(sc.types), R.fptr(sc.records), sc.n, spp, -1)}
    assert all(handles.values())
    rows = {k: {"setup_ms": [], "frame_ms": [], "total_ms": [], "node_visits": [], "prim_tests": []} for k in handles}
    info, images_equal = {}, True
    try:
        for k in handles:  # every handle has rendered once: its workspaces and speculation records exist
            fr.render(handles[k])
        for rep in range(reps + 1):  # the first round is the warm-up
            rec = moved(sc.records, rep)
            shas = {}
            for name in ("recreate", "update_host", "update_device"):
                fr.torch.cuda.synchronize()
                t0 = time.perf_counter()
                if name == "recreate":
                    lib.rt_dev_scene_free(handles[name])
                    handles[name] = lib.rt_dev_scene_iow03(R.fptr(sc.types), R.fptr(rec), sc.n, spp, -1)
                    assert handles[name]
                else:
                    R.update_iow03(handles[name], sc.types, rec, HOST if name == "update_host" else DEVICE)
                setup = (time.perf_counter() - t0) * 1e3
                ms, ctr, sha = fr.render(handles[name])
                shas[name] = sha
                info[name] = R.iow_info(handles[name])
                if rep:
                    r = rows[name]
                    r["setup_ms"].append(setup); r["frame_ms"].append(ms); r["total_ms"].append(setup + ms)
                    r["node_visits"].append(ctr[1]); r["prim_tests"].append(ctr[2])
            images_equal = images_equal and len(set(shas.values())) == 1
    finally:
        for h in handles.values():
            lib.rt_dev_scene_free(h)
    out = {k: {m: mmm(v) for m, v in r.items()} for k, r in rows.items()}
    for k in out:
        out[k]["iow_info"] = info[k]
    a = out["recreate"]["total_ms"]["median"]
    out["ratio_recreate_over_update_host"] = round(a / out["update_host"]["total_ms"]["median"], 4)
    out["ratio_recreate_over_update_device"] = round(a / out["update_device"]["total_ms"]["median"], 4)
    out["images_equal"] = images_equal
    out["reps"] = reps
    return out


def tiled(sc, n):
    """n objects: C2's spheres (every object but the floor) tiled 24 apart in x and z"""
    m = sc.n - 1
    idx, copy = 1 + np.arange(n) % m, np.arange(n) // m
    rec = sc.records[idx].copy()
    rec[:, 0] += (24.0 * (copy % 6)).astype(np.float32)
    rec[:, 2] -= (24.0 * (copy // 6)).astype(np.float32)
    return np.ascontiguousarray(sc.types[idx]), np.ascontiguousarray(rec)


def builder(sc, sizes, reps):
    lib = R.load()
    rows = []
    for n in sizes:
        types, rec = (sc.types[:n], sc.records[:n]) if n <= sc.n else tiled(sc, n)
        types, rec = np.ascontiguousarray(types), np.ascontiguousarray(rec)
        s = lib.rt_dev_scene_iow03(R.fptr(types), R.fptr(rec), n, 1, -1)
        assert s
        t = {HOST: {"build": [], "call": []}, DEVICE: {"build": [], "call": []}}
        info = {}
        try:
            for rep in range(reps + 1):  # the first round is the warm-up
                for flags in (HOST, DEVICE):
                    tm = R.update_iow03(s, types, moved(rec, rep), flags)
                    info[flags] = R.iow_info(s)
                    if rep:
                        t[flags]["build"].append(tm[1]); t[flags]["call"].append(tm[3])
        finally:
            lib.rt_dev_scene_free(s)
        rows.append({"n": n, "host_build_ms": mmm(t[HOST]["build"]), "device_build_ms": mmm(t[DEVICE]["build"]),
                     "host_call_ms": mmm(t[HOST]["call"]), "device_call_ms": mmm(t[DEVICE]["call"]),
                     "host_wide_nodes": info[HOST]["wide_nodes"], "device_wide_nodes": info[DEVICE]["wide_nodes"],
                     "device_built": info[DEVICE]["built"]})
    rule = None
    for r in rows:
        h, d = r["host_build_ms"], r["device_build_ms"]
        if d["median"] < h["median"] - (h["max"] - h["min"]):
            rule = r["n"]
            break
    return {"rows": rows, "reps": reps, "device_build_from_n": rule}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--builder-reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "update_iow.json"))
    ap.add_argument("--width", type=int, default=0)
    ap.add_argument("--height", type=int, default=0)
    ap.add_argument("--spp", type=int, default=0)
    ap.add_argument("--sizes", default="485,1024,2048,4096,16383")
    ap.add_argument("--embed", action="append", default=[])
    a = ap.parse_args()
    over = {k: v for k, v in (("width", a.width), ("height", a.height), ("spp", a.spp)) if v}
    sc = R.make_scene(R.PRESET_IOW03_FINAL, 20250131, 0, **over)
    if R.load().rt_device_info(-1, None, 0, None) != 0:
        raise SystemExit("no gfx950 device: nothing is measured without one")
    res = {"scene": {"preset": "IOW03_FINAL", "seed": 20250131, "objects": sc.n, "width": sc.params.width,
                     "height": sc.params.height, "spp": sc.params.spp, "max_bounces": sc.params.max_bounces},
           "builder": builder(sc, [int(x) for x in a.sizes.split(",")], a.builder_reps),
           "update_vs_recreate": update_vs_recreate(sc, a.reps)}
    u = res["update_vs_recreate"]
    res["tree_quality"] = {k: {"frame_ms": u[k]["frame_ms"], "wide_nodes": u[k]["iow_info"]["wide_nodes"],
                               "lds": u[k]["iow_info"]["lds"], "node_visits": u[k]["node_visits"],
                               "prim_tests": u[k]["prim_tests"]} for k in ("update_host", "update_device")}
    res["tree_quality"]["images_equal"] = u["images_equal"]
    for e in a.embed:
        key, path = e.split("=", 1)
        res[key] = json.load(open(path))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
