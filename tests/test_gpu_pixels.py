"""Pixel queries (rt_camera_rays_async, rt_pixel_query_async, rt_pixels_inw / rt_pixels_iow03) on the
GPU.  All equalities are byte equalities: the camera rays against the fixtures' (tests/path_ref.c and
tests/path_iow_ref.c restate out_Pixel's prologue on the CPU; tests/test_path_ref.py and
tests/test_path_iow_ref.py tie them to the oracle's frames), the pixels against the GPU renders and
the CPU oracle's, the per-sample answers against the fixtures', and the reference's counters."""
import ctypes as C

import numpy as np
import pytest

import path_iow_ref as PI
import path_ref as P
import rt_amd as R
import trace_iow_ref as T

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = 0xCD
INW_COUNTERS = (0, 3, 4, 5)  # segments, shadow queries, dropped pushes, NaN directions: the reference's
IOW_COUNTERS = (0, 4, 5)
STAT_KEYS = ("segments", "node_visits", "prim_tests", "shadow_queries", "stack_drops", "nan_drops")
W, H = P.CAM_W, P.CAM_H
ALL = np.array([(x, y) for y in range(H) for x in range(W)], np.int32)  # the fixtures' (y, x) order

_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def inw_case(name):
    """(fixture, its preset scene with the fixture's bounce limit, the GPU render of its 16 x 9 frame)."""
    def make():
        f = P.load_fixture(name)
        if name == "cam_random600":
            sc = R.make_scene(R.PRESET_INW01_RANDOM, 1234, 600, width=W, height=H, spp=P.SPP)
        else:
            sc = R.make_scene(R.PRESET_INW04_CORNELL, width=W, height=H, spp=P.SPP)
        assert np.array_equal(sc.geom, f.geom)
        assert bytes(sc.camera) == f.camera.tobytes()
        sc.params.max_bounces = f.max_bounces
        return f, sc, R.render(sc)
    return cached(name, make)


def iow_case():
    """(cam_final's fixture, its preset scene)."""
    def make():
        f = PI.load_fixture("cam_final")
        s = T.load_fixture(str(f["scene"]))
        sc = R.make_scene(R.PRESET_IOW03_FINAL, 20250131, 0, width=PI.CAM_W, height=PI.CAM_H, spp=PI.SPP)
        assert np.array_equal(sc.records, s["records"]) and sc.params.max_bounces == f["max_bounces"]
        assert bytes(sc.camera) == f["camera"].tobytes()
        return f, sc
    return cached("cam_final", make)


def up(a):
    """A device copy of the array's bytes, with a spare record behind them."""
    return torch.from_numpy(np.frombuffer(a.tobytes() + bytes(64), np.uint8).copy()).to(torch.device("cuda"))


def rays_async(s, sc, px, s0, ns, tail=3, params=None):
    """rt_camera_rays_async on the current torch stream into a SENTINEL-filled buffer with `tail` records
    to spare.  Returns (rc, records (n + tail,))."""
    iow = sc.stage == R.RT_STAGE_IOW03
    dtype = R.PATH_IOW_RAY_DTYPE if iow else R.PATH_RAY_DTYPE
    px = R.as_pixels(px)
    d_px = up(px)
    d_rays = torch.full(((len(px) * ns + tail) * dtype.itemsize,), SENTINEL, dtype=torch.uint8, device=d_px.device)
    rc = R.load().rt_camera_rays_async(s, C.byref(sc.camera), C.byref(params or sc.params), d_px.data_ptr(), len(px), s0,
                                       ns, d_rays.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, d_rays.cpu().numpy().view(dtype)


def query_async(s, sc, px, samples=True, counters=True, short=0, n_pixels=None, params=None):
    """rt_pixel_query_async on the current torch stream; every output starts as SENTINEL bytes.
    Returns (rc, pixels_out, samples (pixels, spp) or None, counters (6,))."""
    lib = R.load()
    p = params or sc.params
    iow = sc.stage == R.RT_STAGE_IOW03
    dtype = R.PATH_IOW_OUT_DTYPE if iow else R.PATH_OUT_DTYPE
    px = R.as_pixels(px)
    n = len(px) if n_pixels is None else n_pixels
    spp = int(sc.params.spp)  # the scene's
    need = lib.rt_pixel_workspace_bytes(s, len(px))
    assert need >= len(px) * spp * 2 * dtype.itemsize and dtype.itemsize == (48 if iow else 32)
    dev = torch.device("cuda")
    d_px = up(px)
    d_ws = torch.full((max(need, 16),), SENTINEL, dtype=torch.uint8, device=dev)
    d_out = torch.full((max(len(px), 1) * 32,), SENTINEL, dtype=torch.uint8, device=dev)
    d_smp = torch.full((max(len(px), 1) * spp * dtype.itemsize,), SENTINEL, dtype=torch.uint8, device=dev)
    d_ctr = torch.zeros(6, dtype=torch.int64, device=dev)
    rc = lib.rt_pixel_query_async(s, C.byref(sc.camera), C.byref(p), d_px.data_ptr(), n, d_out.data_ptr(),
                                  d_smp.data_ptr() if samples else None, d_ws.data_ptr(), need - short,
                                  d_ctr.data_ptr() if counters else None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    smp = d_smp.cpu().numpy().view(dtype).reshape(-1, spp)
    if not samples:
        assert np.all(smp.view(np.uint8) == SENTINEL)
    return rc, d_out.cpu().numpy().view(R.PIXEL_OUT_DTYPE), smp if samples else None, d_ctr.cpu().numpy()


def same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype.itemsize == want.dtype.itemsize, what
    if got.tobytes() != want.tobytes():
        w = got.dtype.itemsize // 4
        bad = np.flatnonzero((got.reshape(-1).view(np.uint32).reshape(-1, w) !=
                              want.reshape(-1).view(np.uint32).reshape(-1, w)).any(1))
        raise AssertionError(f"{what}: {len(bad)} of {got.size} records differ, first {bad[0]}: got "
                             f"{got.reshape(-1)[bad[0]]} want {want.reshape(-1)[bad[0]]}")


def assert_invalid(recs, what):
    """Every record: sample = 0xffffffff and every other field 0."""
    recs = np.ascontiguousarray(recs).reshape(-1)
    want = np.zeros(len(recs), recs.dtype)
    want["sample"] = 0xFFFFFFFF
    same(recs, want, what)


def image_of(rgba, depth, idx=None):
    """The render's (rgba (P, 4), depth (P,)) at the pixels idx of the (y, x) order; an IOW-03 depth is 0."""
    c = rgba.reshape(-1, 4)
    d = depth.reshape(-1) if depth is not None else np.zeros(len(c), np.float32)
    return (c, d) if idx is None else (c[idx], d[idx])


def assert_pixels(out, rgba, depth, what):
    same(out["rgba"], rgba, what + " rgba")
    same(out["depth"], depth, what + " depth")


# ------------------------------------------------------------------------------ 1, 2: camera rays
@pytest.mark.parametrize("name", P.CAM)
def test_inw_camera_rays(gpu, name):
    f, sc, _ = inw_case(name)
    rays = f.rays.reshape(W * H, P.SPP)
    s = R.dev_scene(sc)
    try:
        rc, got = rays_async(s, sc, ALL, 0, P.SPP)
        assert rc == R.RT_OK
        same(got[:-3], f.rays, f"{name}: all pixels, all samples")
        assert np.all(got[-3:].view(np.uint8) == SENTINEL)  # the tail past n_pixels * ns
        assert not got["pad"][:-3].any()
        # a shuffled list with duplicates, a sample range inside the table
        idx = np.random.default_rng(7).integers(0, W * H, 97)
        rc, got = rays_async(s, sc, ALL[idx], 5, 3)
        assert rc == R.RT_OK
        same(got[:-3], rays[idx, 5:8].reshape(-1), f"{name}: shuffled pixels, samples 5..7")
        assert np.all(got[-3:].view(np.uint8) == SENTINEL)
        # a sample range that overruns the table: two rays, then two invalid records per pixel
        rc, got = rays_async(s, sc, ALL[idx[:5]], 14, 4)
        assert rc == R.RT_OK
        got = got[:-3].reshape(5, 4)
        same(got[:, :2], rays[idx[:5], 14:16], f"{name}: samples 14, 15")
        assert_invalid(got[:, 2:], f"{name}: samples 16, 17")
        # pixels outside the image
        rc, got = rays_async(s, sc, [(-1, 0), (W, 0), (0, H), (3, 2)], 0, P.SPP)
        assert rc == R.RT_OK
        got = got[:-3].reshape(4, P.SPP)
        assert_invalid(got[:3], f"{name}: pixels outside the image")
        same(got[3], rays[2 * W + 3], f"{name}: the pixel after three outside the image")
    finally:
        R.load().rt_dev_scene_free(s)


def test_iow_camera_rays(gpu):
    f, sc = iow_case()
    s = R.dev_scene(sc)
    try:
        rc, got = rays_async(s, sc, ALL, 0, PI.SPP)
        assert rc == R.RT_OK
        same(got[:-3], f["rays"], "cam_final: all pixels, all samples")
        assert np.all(got[-3:].view(np.uint8) == SENTINEL)
        idx = np.random.default_rng(8).integers(0, W * H, 70)
        rc, got = rays_async(s, sc, ALL[idx], 6, 4)  # samples 6, 7, then two past the table
        assert rc == R.RT_OK
        got = got[:-3].reshape(70, 4)
        same(got[:, :2], f["rays"].reshape(-1, PI.SPP)[idx, 6:8], "cam_final: samples 6, 7")
        assert_invalid(got[:, 2:], "cam_final: samples 8, 9")
    finally:
        R.load().rt_dev_scene_free(s)
    same(R.camera_rays(sc, ALL[:5], 2, 3), f["rays"].reshape(-1, PI.SPP)[:5, 2:5].reshape(-1), "rt_amd.camera_rays")


# ------------------------------------------------------------------------------ 3, 4: pixel queries
@pytest.mark.parametrize("name", P.CAM)
def test_inw_pixel_query(gpu, name):
    f, sc, (rgba, depth, st) = inw_case(name)
    inv = P.camera_invert(f.camera)
    want_out = f.out[inv].reshape(W * H, P.SPP)
    s = R.dev_scene(sc)
    try:
        rc, out, smp, ctr = query_async(s, sc, ALL)
        assert rc == R.RT_OK
        assert_pixels(out, *image_of(rgba, depth), name)
        same(smp, want_out, f"{name} samples")
        for k in ("segments", "drops", "nans"):
            assert np.array_equal(out[k], want_out[k].sum(1)), k
        for k in INW_COUNTERS:
            assert int(ctr[k]) == int(st[STAT_KEYS[k]]) == int(f.ctr[inv][k]), k
        order = np.random.default_rng(9).integers(0, W * H, 65)  # shuffled, with duplicates
        for n in (1, 63, 64, 65):
            idx = order[:n]
            rc, out, _, ctr = query_async(s, sc, ALL[idx], samples=False)
            assert rc == R.RT_OK, n
            assert_pixels(out, *image_of(rgba, depth, idx), f"{name}: {n} pixels, samples in the workspace")
            assert int(ctr[0]) == int(want_out["segments"][idx].sum()) and int(ctr[4]) == int(want_out["drops"][idx].sum())
        rc, out, smp, ctr = query_async(s, sc, ALL, counters=False)
        assert rc == R.RT_OK and not ctr.any()
        assert_pixels(out, *image_of(rgba, depth), f"{name}, NULL counters")
        same(smp, want_out, f"{name} samples, NULL counters")
        # pixels outside the image: all-zero records, status 1 samples, nothing counted for them
        rc, out, smp, ctr = query_async(s, sc, [(-1, 0), (3, 2), (W, 0), (0, H)])
        assert rc == R.RT_OK
        assert not out[[0, 2, 3]].view(np.uint8).any()
        assert_pixels(out[1:2], *image_of(rgba, depth, [2 * W + 3]), f"{name}: between pixels outside the image")
        assert np.all(smp["status"][[0, 2, 3]] == 1) and int(ctr[0]) == int(want_out["segments"][2 * W + 3].sum())
    finally:
        R.load().rt_dev_scene_free(s)


@pytest.mark.parametrize("spec", [1, 0])
def test_iow_pixel_query(gpu, spec):
    f, sc = iow_case()
    with R.options(iow_spec=spec):
        rgba, depth, st = R.render(sc)
    want_out = f["out"].reshape(W * H, PI.SPP)
    s = R.dev_scene(sc)
    try:
        rc, out, smp, ctr = query_async(s, sc, ALL)
        rc2, out2, _, _ = query_async(s, sc, [(W, 1), (5, 4), (2, -1)])
    finally:
        R.load().rt_dev_scene_free(s)
    assert rc == R.RT_OK and rc2 == R.RT_OK
    assert not out2[[0, 2]].view(np.uint8).any()  # pixels outside the image
    assert_pixels(out2[1:2], *image_of(rgba, depth, [4 * W + 5]), "cam_final: between pixels outside the image")
    assert_pixels(out, *image_of(rgba, depth), f"cam_final against the render, iow_spec {spec}")
    same(PI.canon(smp.reshape(-1)), PI.canon(f["out"]), "cam_final samples")
    for k in ("segments", "drops", "nans"):
        assert np.array_equal(out[k], want_out[k].sum(1)), k
    for k, v in zip(IOW_COUNTERS, f["ctr"]):
        assert int(ctr[k]) == int(st[STAT_KEYS[k]]) == int(v), k
    assert int(ctr[3]) == 0


# ------------------------------------------------------------------------------ 5: odd sizes, the oracle
ODD = {"inw01": lambda: R.make_scene(R.PRESET_INW01_RANDOM, 1234, 600, width=37, height=23, spp=5, max_bounces=8),
       "inw04": lambda: R.make_scene(R.PRESET_INW04_CORNELL, width=23, height=37, spp=3),
       "iow03": lambda: R.make_scene(R.PRESET_IOW03_FINAL, 20250131, 0, width=37, height=23, spp=5, max_bounces=6),
       # more samples than a wave has lanes: the fold takes a pixel's answers 64 at a time (three rounds,
       # two, two; the last one ragged; INW's depth sample spp / 2 in the second round)
       "inw01_spp130": lambda: R.make_scene(R.PRESET_INW01_RANDOM, 1234, 600, width=9, height=5, spp=130,
                                            max_bounces=8),
       "inw04_spp67": lambda: R.make_scene(R.PRESET_INW04_CORNELL, width=5, height=9, spp=67),
       "iow03_spp70": lambda: R.make_scene(R.PRESET_IOW03_FINAL, 20250131, 0, width=9, height=5, spp=70,
                                           max_bounces=6)}


@pytest.mark.parametrize("case", list(ODD))
def test_odd_sizes_against_the_oracle(gpu, case):
    """Frames whose width and height are no multiple of 8 or 64 and whose spp divides neither 64 nor the
    chain claims (and is odd: the depth sample is spp / 2 rounded down), through the blocking forms."""
    from oracle import oracle as O
    sc = ODD[case]()
    p = sc.params
    orgba, odepth, ost = O.render(sc, p)
    px = np.array([(x, y) for y in range(p.height) for x in range(p.width)], np.int32)
    res = R.pixels(sc, px, want_rays=True, want_samples=True)
    out, st = res["pixels"], res["stats"]
    assert_pixels(out, *image_of(orgba, odepth), case)
    for k in ("segments", "shadow_queries", "stack_drops", "nan_drops"):
        assert st[k] == ost[k], k
    smp = res["samples"]
    assert smp.shape == (len(px), p.spp) and not smp["status"].any()
    assert np.array_equal(out["segments"], smp["segments"].sum(1)) and int(out["segments"].sum()) == ost["segments"]
    assert int(out["drops"].sum()) == ost["stack_drops"] and int(out["nans"].sum()) == ost["nan_drops"]
    assert np.array_equal(res["rays"]["sample"], np.tile(np.arange(p.spp, dtype=np.uint32), (len(px), 1)))
    same(res["rays"].reshape(-1), R.camera_rays(sc, px), f"{case}: the blocking form's rays")


# ------------------------------------------------------------------------------ 6: options and updates
@pytest.mark.parametrize("option", ["inw_wide_walk", "inw_time_bins", "inw_sphere_records", "inw_fused_cull"])
def test_options_do_not_change_results(gpu, option):
    f, sc, (rgba, depth, st) = inw_case("cam_random600")
    inv = P.camera_invert(f.camera)
    with R.options(**{option: 0}):
        s = R.dev_scene(sc)  # a scene keeps the options it was created with
    try:
        rc, out, smp, ctr = query_async(s, sc, ALL)
    finally:
        R.load().rt_dev_scene_free(s)
    assert rc == R.RT_OK
    assert_pixels(out, *image_of(rgba, depth), f"{option} = 0")
    same(smp.reshape(-1), f.out[inv], f"{option} = 0 samples")
    for k in INW_COUNTERS:
        assert int(ctr[k]) == int(f.ctr[inv][k]), k


def glass_scene(name):
    """The glass600 / glass600_b fixture's objects as a Scene seen from the side of their slab."""
    f = P.load_fixture(name)
    cam = R.RtCamera()
    cam.pos[:] = (0.0, 4.0, 30.0)
    d = np.array([0.0, -0.1, -1.0])
    cam.dir[:] = [float(v) for v in (d / np.linalg.norm(d)).astype(np.float32)]
    cam.fov_y_rad, cam.aperture, cam.focus_dist = 0.8, 0.1, 25.0
    p = R.RtParams(width=W, height=H, spp=f.spp, max_bounces=f.max_bounces, device=-1)
    assert f.layout == 1 and f.n_lights == 0
    return R.Scene(stage=R.RT_STAGE_INW01, desc=None, n=f.n, camera=cam, params=p, geom=f.geom, aabbs=f.aabbs,
                   nodes=f.nodes)


@pytest.mark.parametrize("device_build", [False, True])
def test_updated_scene_answers_as_the_new_frame(gpu, device_build):
    a, b = glass_scene("glass600"), glass_scene("glass600_b")
    lib = R.load()

    def fresh():
        s = R.dev_scene(b)
        try:
            return query_async(s, b, ALL)
        finally:
            lib.rt_dev_scene_free(s)

    rc, want, want_smp, want_ctr = cached("glass600_b fresh", fresh)
    assert rc == R.RT_OK and want_smp["segments"].sum() > 2 * want_smp.size  # the view sees the glass
    s = R.dev_scene(a)
    try:
        rc = lib.rt_dev_scene_inw_update(s, R.fptr(b.geom), b.n, None if device_build else R.fptr(b.nodes),
                                         R.fptr(b.aabbs) if device_build else None, None, 0, None)
        assert rc == R.RT_OK
        rc, out, smp, ctr = query_async(s, b, ALL)
    finally:
        lib.rt_dev_scene_free(s)
    assert rc == R.RT_OK
    same(out, want, "updated scene pixels")
    same(smp, want_smp, "updated scene samples")
    for k in INW_COUNTERS:
        assert int(ctr[k]) == int(want_ctr[k]), k


# ------------------------------------------------------------------------------ 7: errors on a device
def test_errors_on_a_device(gpu):
    f, sc, (rgba, depth, _) = inw_case("cam_random600")
    s = R.dev_scene(sc)

    def untouched(rc, out, smp, ctr, want):
        assert rc == want
        assert np.all(out.view(np.uint8) == SENTINEL) and np.all(smp.view(np.uint8) == SENTINEL) and not ctr.any()

    def params(**kw):
        p = R.RtParams.from_buffer_copy(sc.params)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    try:
        untouched(*query_async(s, sc, ALL[:4], params=params(spp=8)), R.RT_E_ARG)       # not the scene's spp
        assert rays_async(s, sc, ALL[:4], 0, 4, params=params(spp=8))[0] == R.RT_E_ARG
        untouched(*query_async(s, sc, ALL[:4], params=params(show_normal=1)), R.RT_E_UNSUPPORTED)
        untouched(*query_async(s, sc, ALL[:4], short=1), R.RT_E_ARG)                     # a byte short
        untouched(*query_async(s, sc, ALL[:4], n_pixels=0), R.RT_OK)                     # nothing launched
        rc, got = rays_async(s, sc, ALL[:4], 0, 0)
        assert rc == R.RT_OK and np.all(got.view(np.uint8) == SENTINEL)
        rc, out, _, _ = query_async(s, sc, ALL[:4])                                      # and the scene still answers
        assert rc == R.RT_OK
        assert_pixels(out, *image_of(rgba, depth, np.arange(4)), "after the errors")
    finally:
        R.load().rt_dev_scene_free(s)


# ------------------------------------------------------------------------------ 8: graph capture
@pytest.mark.parametrize("family", ["inw", "iow"])
def test_graph_capture(gpu, family):
    """One call captured in a graph (memsets and kernels on one stream: a single branch), replayed twice:
    the eager bytes both times, the counters added twice."""
    if family == "inw":
        f, sc, _ = inw_case("cam_random600")
    else:
        f, sc = iow_case()
    lib = R.load()
    dev = torch.device("cuda")
    s = R.dev_scene(sc)
    try:
        rc, want, want_smp, want_ctr = query_async(s, sc, ALL)
        assert rc == R.RT_OK
        need = lib.rt_pixel_workspace_bytes(s, len(ALL))
        d_px = up(R.as_pixels(ALL))
        d_ws = torch.zeros(need, dtype=torch.uint8, device=dev)
        d_out = torch.full((want.nbytes,), SENTINEL, dtype=torch.uint8, device=dev)
        d_smp = torch.full((want_smp.nbytes,), SENTINEL, dtype=torch.uint8, device=dev)
        d_ctr = torch.zeros(6, dtype=torch.int64, device=dev)

        def call():
            return lib.rt_pixel_query_async(s, C.byref(sc.camera), C.byref(sc.params), d_px.data_ptr(), len(ALL),
                                            d_out.data_ptr(), d_smp.data_ptr(), d_ws.data_ptr(), need, d_ctr.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream)

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):  # once outside the capture (the occupancy query runs here)
            assert call() == R.RT_OK
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        d_ctr.zero_()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            assert call() == R.RT_OK
        for k in (1, 2):
            d_out.fill_(SENTINEL)
            d_smp.fill_(SENTINEL)
            graph.replay()
            torch.cuda.synchronize()
            same(d_out.cpu().numpy().view(R.PIXEL_OUT_DTYPE), want, f"replay {k} pixels")
            same(d_smp.cpu().numpy().view(want_smp.dtype), want_smp.reshape(-1), f"replay {k} samples")
            got = d_ctr.cpu().numpy()
            for c in (INW_COUNTERS if family == "inw" else IOW_COUNTERS):
                assert int(got[c]) == k * int(want_ctr[c]), (k, c)
        del graph
    finally:
        torch.cuda.synchronize()
        lib.rt_dev_scene_free(s)


# ------------------------------------------------------------------------------ 9: resources
def test_kernel_resources(gpu):
    """The kernels as loaded: no scratch, no LDS, and the registers of DESIGN.md 5.11's table."""
    table = {0: 30, 1: 33, 2: 40, 3: 26}
    for which, vgprs in table.items():
        info = R.pixels_kernel_info(which)
        print(R.PIXELS_KERNELS[which], info)
        assert info["scratch_bytes"] == 0 and info["lds_bytes"] == 0
        assert info["vgprs"] == vgprs
        assert info["blocks_per_cu"] >= 1
