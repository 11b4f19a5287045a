"""Times of the adaptive sample passes (rt_render_pass_pixels_async, rt_pass_select_async) at workload size.

  c3  the bench scene (In-Next-Week 01, 10k moving spheres, seed 1234, 1920x1080, 500 spp, 50 bounces),
      batches of --samples-c3 samples (16)
  c2  the IOW-03 final scene (1200x800, 100 spp), batches of --samples-c2 samples (10)

For each scene:
  full_list   a listed pass over every pixel, in the order rt_pass_select_async lists them, alternating with
              rt_render_pass_async for the same samples (c3: s0 = 0 and s0 = 240; c2: s0 = 0): the ratio and
              the spread of the alternating runs
  partial     listed passes over about 50%, 10% and 1% of the pixels (a random subset, compacted by
              rt_pass_select_async) from count 0, beside that fraction of the full-list time
  select      rt_pass_select_async beside a hipMemsetAsync of the bytes it reads and writes once (16 B of
              state, 16 B of aux, 8 B of list, 4 B of err per pixel)
  loop        the whole loop (pass + select + the read-back of n_active per round) at two tolerances, the
              median and the 90th percentile of the error image after the first round: rounds, samples
              rendered against W * H * spp, time against rt_render_image_async and against all-uniform
              passes of the same batch (c2: one run each, c3: --loop-reps; the runs of a loop are
              deterministic, so the rounds and sample counts reported are those of every run and only the
              time is a median)
  exactness   tol = -1: the last pass's image, depth and the summed counters against the frame's

Every time: HIP events around each call, 3 warm-up launches, then --reps timed ones; median [min, max].
Prints one JSON line per scene (and writes it to --out-c3 / --out-c2).  Needs an MI355X.
    python tools/adaptive_bench.py [--scene c3|c2|both] [--out-c3 profiles/adaptive_c3.json] [--out-c2 ...]
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


def stream():
    return torch.cuda.current_stream().cuda_stream


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


def alternate(f_list, f_pass, reps, pre=None):
    """The listed pass and the uniform pass timed in turn, twice each; the spread of the alternating runs is
    the larger of the two differences between a measurement's medians."""
    l1, p1 = timed(f_list, reps, pre=pre), timed(f_pass, reps)
    l2, p2 = timed(f_list, reps, pre=pre), timed(f_pass, reps)
    spread = max(abs(l1["ms_median"] - l2["ms_median"]), abs(p1["ms_median"] - p2["ms_median"]))
    lm, pm = min(l1["ms_median"], l2["ms_median"]), min(p1["ms_median"], p2["ms_median"])
    return {"listed": {**l1, "again": l2}, "uniform": {**p1, "again": p2}, "spread_ms": round(spread, 4),
            "listed_over_uniform": round(lm / pm, 4), "difference_ms": round(lm - pm, 4),
            "verdict": "within the spread" if abs(lm - pm) <= spread else "OUTSIDE THE SPREAD"}


class Frame:
    """The device buffers of one frame's passes, listed passes and selects."""

    def __init__(self, lib, scene, sc, dev):
        self.lib, self.scene, self.sc, self.dev = lib, scene, sc, dev
        p = sc.params
        self.n = n = p.width * p.height
        self.state = torch.zeros((n, 8), dtype=torch.float32, device=dev)
        self.aux = torch.zeros((n, 4), dtype=torch.int32, device=dev)
        self.rgba = torch.zeros((n, 4), dtype=torch.float32, device=dev)
        self.depth = torch.zeros(n, dtype=torch.float32, device=dev)
        self.err = torch.zeros(n, dtype=torch.float32, device=dev)
        self.list = torch.zeros((n, 2), dtype=torch.int32, device=dev)
        self.n_active = torch.zeros(4, dtype=torch.int32, device=dev)
        self.ctr = torch.zeros(6, dtype=torch.int64, device=dev)

    def uniform(self, s0, ns, counters=False):
        sc = self.sc
        ok(self.lib.rt_render_pass_async(self.scene, C.byref(sc.camera), C.byref(sc.params), s0, ns,
                                         self.state.data_ptr(), self.rgba.data_ptr(), self.depth.data_ptr(),
                                         self.ctr.data_ptr() if counters else None, stream()), "rt_render_pass_async")

    def listed(self, n_pixels, ns, counters=False, lst=None):
        sc = self.sc
        ok(R.pass_pixels(self.scene, sc.camera, sc.params, self.list if lst is None else lst, n_pixels, ns, self.state,
                         self.aux, self.rgba, self.depth, self.ctr if counters else None, stream()),
           "rt_render_pass_pixels_async")

    def select(self, tol, min_samples=2, err=True):
        ok(R.pass_select(self.scene, self.sc.params, self.state, self.aux, tol, min_samples, self.list, self.n_active,
                         self.err if err else None, stream()), "rt_pass_select_async")

    def active(self):
        return int(self.n_active[0].item())  # synchronises: the loop's read-back

    def counts(self):
        return self.aux[:, 3]

    def loop(self, batch, tol, counters=False):
        """The blocking forms' loop from a zeroed aux buffer: (rounds, device ms summed over the rounds)."""
        self.aux.zero_()
        self.select(-1.0, 0, err=False)
        n, rounds, ev = self.active(), 0, []
        while n > 0:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            self.listed(n, batch, counters)
            self.select(tol)
            b.record()
            n = self.active()
            ev.append((a, b))
            rounds += 1
        return rounds, sum(a.elapsed_time(b) for a, b in ev)


def render(lib, scene, sc, dev, reps):
    """rt_render_image_async of the frame: (rgba, depth, counters, timing)."""
    p = sc.params
    n = p.width * p.height
    rgba = torch.zeros((n, 4), dtype=torch.float32, device=dev)
    depth = torch.zeros(n, dtype=torch.float32, device=dev)
    ctr = torch.zeros(6, dtype=torch.int64, device=dev)

    def go(c=None):
        ok(lib.rt_render_image_async(scene, C.byref(sc.camera), C.byref(p), rgba.data_ptr(), depth.data_ptr(), c,
                                     stream()), "rt_render_image_async")

    go(ctr.data_ptr())
    torch.cuda.synchronize()
    return rgba, depth, [int(v) for v in ctr.cpu().tolist()], timed(go, reps, warm=1)


def measure(lib, dev, sc, a, ns, starts, slots, iow, loop_reps):
    p = sc.params
    spp, npx = int(p.spp), p.width * p.height
    scene = R.dev_scene(sc, device=0)
    res = {}
    try:
        fr = Frame(lib, scene, sc, dev)
        fr.select(-1.0, 0, err=False)       # every pixel, in the units' order
        assert fr.active() == npx
        full = fr.list.clone()
        # ---- the full list against the uniform pass
        res["full_list"] = []
        full_ms = None
        for s0 in starts:
            saved = torch.zeros_like(fr.aux)
            saved[:, 3] = s0

            def pre():
                fr.aux.copy_(saved)

            r = alternate(lambda: fr.listed(npx, ns, lst=full), lambda: fr.uniform(s0, ns), a.reps, pre=pre)
            res["full_list"].append({"s0": s0, "ns": ns, **r})
            if s0 == 0:
                full_ms = min(r["listed"]["ms_median"], r["listed"]["again"]["ms_median"])
        # ---- partial lists from count 0
        res["partial"] = []
        rng = torch.Generator(device="cpu").manual_seed(1234)
        for frac in (0.5, 0.1, 0.01):
            done = (torch.rand(npx, generator=rng) >= frac).to(dev)
            saved = torch.zeros_like(fr.aux)
            saved[done, 3] = spp            # at S: inactive
            fr.aux.copy_(saved)
            fr.select(-1.0, 0, err=False)
            n = fr.active()
            lst = fr.list.clone()
            t = timed(lambda: fr.listed(n, ns, lst=lst), a.reps, pre=lambda: fr.aux.copy_(saved))
            res["partial"].append({"fraction_asked": frac, "pixels": n, "fraction": round(n / npx, 5), **t,
                                   "fraction_of_full_list_ms": round(full_ms * n / npx, 4),
                                   "over_that": round(t["ms_median"] / (full_ms * n / npx), 3)})
        # ---- select beside a memset of its bytes
        fr.aux.zero_()
        fr.listed(npx, ns, lst=full)
        torch.cuda.synchronize()
        yard = torch.empty(npx * 44, dtype=torch.uint8, device=dev)
        hip = hip_runtime()
        sel = timed(lambda: fr.select(0.01), a.reps)
        mem = timed(lambda: ok(hip.hipMemsetAsync(yard.data_ptr(), 0, npx * 44, stream()), "hipMemsetAsync"), a.reps)
        tbs = lambda t: round(npx * 44 / t["ms_median"] / 1e9, 3)  # noqa: E731
        res["select"] = {"select": sel, "hipMemsetAsync_44B_per_pixel": mem, "bytes": npx * 44,
                         "select_TB_per_s": tbs(sel), "memset_TB_per_s": tbs(mem),
                         "select_over_memset": round(sel["ms_median"] / mem["ms_median"], 3), "launches": 3}
        first_err = fr.err.cpu().numpy()
        del yard
        # ---- the frame, the all-uniform passes, the exactness of tol = -1
        want = render(lib, scene, sc, dev, 3 if iow else 5)
        if iow:
            want = (want[0], torch.zeros_like(want[1]), want[2], want[3])  # a pass writes the depth 0
        fr.ctr.zero_()
        rounds, ms = fr.loop(ns, -1.0, counters=True)
        got = [int(v) for v in fr.ctr.cpu().tolist()]
        res["exactness"] = {"tol": -1.0, "rounds": rounds, "loop_ms": round(ms, 4),
                            "rgba_equal_render": bool(torch.equal(fr.rgba.view(torch.int32), want[0].view(torch.int32))),
                            "depth_equal_render": bool(torch.equal(fr.depth.view(torch.int32), want[1].view(torch.int32))),
                            "counters_equal_render": all(got[k] == want[2][k] for k in slots),
                            "all_counts_equal_spp": bool((fr.counts() == spp).all().item())}

        def uniform_frame():
            for s0 in range(0, spp, ns):
                fr.uniform(s0, ns)

        uni = timed(uniform_frame, loop_reps, warm=0 if iow else 1)
        res["context"] = {"frame": want[3], "all_uniform_passes": uni, "passes": -(-spp // ns)}
        # ---- the whole loop at two tolerances
        finite = first_err[np.isfinite(first_err)]
        res["loop"] = []
        for pct in (50, 90):
            tol = float(np.percentile(finite, pct))
            runs = [fr.loop(ns, tol) for _ in range(loop_reps)]
            ms = sorted(r[1] for r in runs)[len(runs) // 2]
            samples = int(fr.counts().to(torch.int64).sum().item())
            cnt = fr.counts().cpu().numpy()
            res["loop"].append({"tol_percentile_of_first_round_err": pct, "tol": tol, "rounds": runs[0][0],
                                "loop_ms": round(ms, 4), "runs": len(runs), "samples": samples,
                                "samples_over_full": round(samples / (npx * spp), 4),
                                "pixels_at_first_batch": round(float((cnt <= ns).mean()), 4),
                                "pixels_at_spp": round(float((cnt >= spp).mean()), 4),
                                "over_frame": round(ms / want[3]["ms_median"], 4),
                                "over_all_uniform_passes": round(ms / uni["ms_median"], 4)})
    finally:
        torch.cuda.synchronize()
        lib.rt_dev_scene_free(scene)
    which = (10, 11) if iow else (8, 9)
    return {"objects": sc.n, "frame": [p.width, p.height], "spp": spp, "max_bounces": int(p.max_bounces), "batch": ns,
            **res, "kernels": {R.ADAPTIVE_KERNELS[i]: R.pass_kernel_info(i) for i in which + (12, 13, 14)}}


def bench_c3(lib, dev, a):
    sc = R.make_scene(R.PRESET_INW01_RANDOM, 1234, 10_000, width=1920, height=1080, spp=500)
    return {"tool": "tools/adaptive_bench.py", "scene": "C3: In-Next-Week 01, 10k moving spheres (seed 1234)",
            **measure(lib, dev, sc, a, a.samples_c3, (0, 240), (0, 3, 4, 5), False, a.loop_reps)}


def bench_c2(lib, dev, a):
    sc = R.make_scene(R.PRESET_IOW03_FINAL, 20250131, 0)
    return {"tool": "tools/adaptive_bench.py", "scene": "C2: In-One-Weekend 03 final scene (seed 20250131)",
            **measure(lib, dev, sc, a, a.samples_c2, (0,), (0, 4, 5), True, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", choices=("c3", "c2", "both"), default="both")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--loop-reps", type=int, default=3)
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
