"""rt_dev_scene_iow03_update_device measured against rt_dev_scene_iow03_update, one
process, warm-up first, the arms alternating call by call, medians with [min, max].

At each size (the C2 records, 486 objects, and C2's spheres tiled to 1455 and 16383 objects) an edit moves
every object, on the device for the device arms (before the clock starts) and in a host array for the
host-pointer arms:

  device_DEVICE, device_0   rt_dev_scene_iow03_update_device with RT_UPDATE_DEVICE_BUILD and with flags = 0
  host_DEVICE, host_0       rt_dev_scene_iow03_update with the same flags, fed from host arrays: what a
                            device-resident producer pays today, once cpu_copy is added
  cpu_copy                  the producer's .cpu() of the types and records (n * 25 floats), synchronised

At 486 objects the C2 frame (1200 x 800, 100 spp) that follows each update is timed too.

python tools/prof_update_iow_dev.py [--reps 15] [--frame-reps 5] [--out profiles/update_iow_dev.json]
                                    [--width W --height H --spp S]   (a smaller frame, for a rehearsal)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "raytracing-tests_amd"), os.path.join(ROOT, "tools")]
import rt_amd as R  # noqa: E402
from prof_update_iow import Frames, mmm, tiled  # noqa: E402

DEVICE = R.RT_UPDATE_DEVICE_BUILD
ARMS = (("device_DEVICE", True, DEVICE), ("host_DEVICE", False, DEVICE), ("device_0", True, 0), ("host_0", False, 0))


def delta_of(n, k):
    """edit number k of n objects: every object moves (the offsets alternate, so edits never repeat)"""
    d = np.zeros((n, 24), np.float32)
    i = np.arange(n)
    for a in range(3):
        d[:, a] = 0.02 * (k % 2 + 1) * ((i + a) % 3 - 1)
    return d


def measure(sc, types, rec, reps, frames):
    """One size: every arm on a scene handle of its own, `reps` measured rounds after one warm-up round."""
    import torch
    lib = R.load()
    dev = torch.device("cuda")
    n = len(types)
    spp = sc.params.spp if frames else 1
    handles = {name: lib.rt_dev_scene_iow03(R.fptr(types), R.fptr(rec), n, spp, -1) for name, _, _ in ARMS}
    assert all(handles.values())
    d_types = torch.from_numpy(types).to(dev)
    d_base = torch.from_numpy(rec.reshape(-1)).to(dev)
    rows = {name: {"call_ms": [], "timing_ms": [], "frame_ms": [], "total_ms": []} for name, _, _ in ARMS}
    copy_ms, info, shas_equal = [], {}, True
    fr = Frames(sc) if frames else None
    st = torch.cuda.current_stream().cuda_stream
    try:
        if fr:
            for h in handles.values():  # every handle has rendered once: its workspaces exist
                fr.render(h)
        for rep in range(reps + 1):  # the first round is the warm-up
            d = delta_of(n, rep)
            host_rec = np.ascontiguousarray(rec + d)
            d_rec = d_base + torch.from_numpy(d.reshape(-1)).to(dev)  # the edit, on the device
            torch.cuda.synchronize()
            assert np.array_equal(d_rec.cpu().numpy().reshape(n, 24), host_rec)
            t0 = time.perf_counter()
            back = (d_types.cpu(), d_rec.cpu())  # .cpu() of a device tensor returns when the copy is done
            if rep:
                copy_ms.append((time.perf_counter() - t0) * 1e3)
            del back
            shas = {}
            for name, on_device, flags in ARMS:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if on_device:
                    tm = R.update_iow03_device(handles[name], d_types, d_rec, n, flags, stream=st)
                else:
                    tm = R.update_iow03(handles[name], types, host_rec, flags)
                call = (time.perf_counter() - t0) * 1e3
                info[name] = R.iow_info(handles[name])
                ms = 0.0
                if fr:
                    ms, _, shas[name] = fr.render(handles[name])
                if rep:
                    r = rows[name]
                    r["call_ms"].append(call); r["timing_ms"].append(tm)
                    if fr:
                        r["frame_ms"].append(ms); r["total_ms"].append(call + ms)
            shas_equal = shas_equal and len(set(shas.values())) <= 1
    finally:
        for h in handles.values():
            lib.rt_dev_scene_free(h)
    out = {"n": n, "reps": reps, "cpu_copy_ms": mmm(copy_ms)}
    for name, r in rows.items():
        o = {"call_ms": mmm(r["call_ms"]), "built": info[name]["built"], "wide_nodes": info[name]["wide_nodes"],
             "timing_ms": [mmm([t[k] for t in r["timing_ms"]]) for k in range(4)]}
        if fr:
            o["frame_ms"], o["total_ms"] = mmm(r["frame_ms"]), mmm(r["total_ms"])
        out[name] = o
    for flag in ("DEVICE", "0"):
        out[f"host_{flag}_plus_copy_ms"] = round(out[f"host_{flag}"]["call_ms"]["median"] + out["cpu_copy_ms"]["median"], 4)
    if fr:
        out["images_equal"] = shas_equal
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--frame-reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "update_iow_dev.json"))
    ap.add_argument("--width", type=int, default=0)
    ap.add_argument("--height", type=int, default=0)
    ap.add_argument("--spp", type=int, default=0)
    ap.add_argument("--sizes", default="1455,16383")
    a = ap.parse_args()
    over = {k: v for k, v in (("width", a.width), ("height", a.height), ("spp", a.spp)) if v}
    sc = R.make_scene(R.PRESET_IOW03_FINAL, 20250131, 0, **over)
    if R.load().rt_device_info(-1, None, 0, None) != 0:
        raise SystemExit("no gfx950 device: nothing is measured without one")
    c2 = (np.ascontiguousarray(sc.types, np.float32), np.ascontiguousarray(sc.records, np.float32))
    res = {"scene": {"preset": "IOW03_FINAL", "seed": 20250131, "objects": sc.n, "width": sc.params.width,
                     "height": sc.params.height, "spp": sc.params.spp, "max_bounces": sc.params.max_bounces},
           "kernels": {name: R.update_iow_kernel_info(k) for k, name in enumerate(R.UPDATE_IOW_KERNELS)},
           "updates": [measure(sc, *c2, a.reps, False)] + [measure(sc, *tiled(sc, int(n)), a.reps, False)
                                                           for n in a.sizes.split(",") if n],
           "update_and_frame_c2": measure(sc, *c2, a.frame_reps, True)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
