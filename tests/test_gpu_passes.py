"""Progressive sample passes (rt_render_pass_async, rt_render_passes_inw / rt_render_passes_iow03) on the
GPU.  Every equality is a byte equality: the last pass against rt_render_image_async of the same handle,
every intermediate state and image against tests/pass_ref.py (prefix folds over the path-query
fixtures; tests/test_pass_ref.py ties them to the oracle's frames), the blocking forms against the CPU
oracle, and the reference's counters summed over the passes against the render's."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import pass_ref as PR
import path_iow_ref as PI
import path_ref as P
import rt_amd as R
import trace_iow_ref as T

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = 0xCD
INW_COUNTERS = (0, 3, 4, 5)  # segments, shadow queries, dropped pushes, NaN directions: the reference's
IOW_COUNTERS = (0, 4, 5)
W, H = PR.W, PR.H
# a pass begins at, ends at and straddles spp / 2 = 8 of the 16-spp INW fixtures
CUTS = [(16,), tuple(range(1, 17)), (3, 8, 16), (8, 16), (9, 16)]
# cam_final has 8 spp: the same cuts with every pass asking for its full range (the passes that reach spp
# are clipped there and end the frame), and the three that begin at, end at and straddle its spp / 2 = 4
IOW_CUTS = CUTS + [(4, 8), (5, 8), (2, 4, 8)]

_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def scene_of(name):
    """The preset scene of a camera fixture, with the fixture's bounce limit."""
    def make():
        if name == PR.IOW:
            f = PI.load_fixture(name)
            sc = R.make_scene(R.PRESET_IOW03_FINAL, 20250131, 0, width=W, height=H, spp=PI.SPP)
            assert np.array_equal(sc.records, T.load_fixture(str(f["scene"]))["records"])
            assert bytes(sc.camera) == f["camera"].tobytes() and sc.params.max_bounces == f["max_bounces"]
            return sc
        f = P.load_fixture(name)
        if name == "cam_random600":
            sc = R.make_scene(R.PRESET_INW01_RANDOM, 1234, 600, width=W, height=H, spp=P.SPP)
        else:
            sc = R.make_scene(R.PRESET_INW04_CORNELL, width=W, height=H, spp=P.SPP)
        assert np.array_equal(sc.geom, f.geom) and bytes(sc.camera) == f.camera.tobytes()
        sc.params.max_bounces = f.max_bounces
        return sc
    return cached(("scene", name), make)


def is_iow(sc):
    return sc.stage == R.RT_STAGE_IOW03


def counter_slots(sc):
    return IOW_COUNTERS if is_iow(sc) else INW_COUNTERS


def params_of(sc, **kw):
    p = R.RtParams.from_buffer_copy(sc.params)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def filled(nbytes):
    return torch.full((max(nbytes, 16),), SENTINEL, dtype=torch.uint8, device=torch.device("cuda"))


def render_async(s, sc, params=None):
    """rt_render_image_async into SENTINEL-filled buffers: (rgba (H*W, 4), depth (H*W,), counters (6,))."""
    p = params or sc.params
    n = p.width * p.height
    d_rgba, d_depth = filled(n * 16), filled(n * 4)
    d_ctr = torch.zeros(6, dtype=torch.int64, device=d_rgba.device)
    rc = R.load().rt_render_image_async(s, C.byref(sc.camera), C.byref(p), d_rgba.data_ptr(), d_depth.data_ptr(),
                                        d_ctr.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == R.RT_OK
    return (d_rgba.cpu().numpy()[: n * 16].view(np.float32).reshape(n, 4), d_depth.cpu().numpy()[: n * 4].view(np.float32),
            d_ctr.cpu().numpy())


class Passes:
    """The buffers of one frame's passes, all SENTINEL bytes at first, and the frame's counters."""

    def __init__(self, s, sc, params=None, rgba=True, depth=True, counters=True):
        self.s, self.sc, self.p = s, sc, params or sc.params
        self.n = self.p.width * self.p.height
        self.d_state = filled(self.n * 32)
        self.d_rgba = filled(self.n * 16) if rgba else None
        self.d_depth = filled(self.n * 4) if depth else None
        self.d_ctr = torch.zeros(6, dtype=torch.int64, device=self.d_state.device) if counters else None

    def call(self, s0, ns, params=None):
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        return R.load().rt_render_pass_async(self.s, C.byref(self.sc.camera), C.byref(params or self.p), s0, ns,
                                             ptr(self.d_state), ptr(self.d_rgba), ptr(self.d_depth), ptr(self.d_ctr),
                                             torch.cuda.current_stream().cuda_stream)

    def run(self, s0, ns, params=None):
        rc = self.call(s0, ns, params)
        torch.cuda.synchronize()
        return rc

    def state(self):
        return self.d_state.cpu().numpy()[: self.n * 32].view(R.PASS_STATE_DTYPE)

    def rgba(self):
        return self.d_rgba.cpu().numpy()[: self.n * 16].view(np.float32).reshape(self.n, 4)

    def depth(self):
        return self.d_depth.cpu().numpy()[: self.n * 4].view(np.float32)

    def counters(self):
        return self.d_ctr.cpu().numpy()


def same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype.itemsize == want.dtype.itemsize, what
    if got.tobytes() != want.tobytes():
        w = got.dtype.itemsize // 4
        g = got.reshape(-1).view(np.uint32).reshape(-1, w)
        bad = np.flatnonzero((g != want.reshape(-1).view(np.uint32).reshape(-1, w)).any(1))
        raise AssertionError(f"{what}: {len(bad)} of {len(g)} records differ, first {bad[0]}: got "
                             f"{got.reshape(-1)[bad[0]]} want {want.reshape(-1)[bad[0]]}")


def same_state(got, want, iow, what):
    """States bit for bit: on IOW-03 all 32 bytes; on INW acc and depth, with ri left as SENTINEL bytes."""
    same(got["acc"], want["acc"], what + " acc")
    same(got["depth"], want["depth"], what + " depth")
    if iow:
        same(got["ri"], want["ri"], what + " ri")
    else:
        assert np.all(got["ri"].view(np.uint8) == SENTINEL), what + ": ri is neither read nor written"


def run_cuts(ps, cuts, spp, name=None, m=slice(None)):
    """The passes of `cuts`, each asking for its full range (clipped at spp), until one reaches spp; after
    each pass, with `name`, the state and image (of the pixels m) against pass_ref.  Returns the samples
    rendered."""
    iow = is_iow(ps.sc)
    s0 = 0
    for c in cuts:
        assert ps.run(s0, c - s0) == R.RT_OK, (s0, c)
        k = min(c, spp)
        if name:
            want = PR.state(name, k)
            same_state(ps.state()[m], want[m], iow, f"{name}: state after {k} samples")
            rgba, depth = PR.image(want, k)
            same(ps.rgba()[m], rgba[m], f"{name}: image after {k} samples")
            same(ps.depth()[m], depth[m], f"{name}: depth after {k} samples")
            if not iow and k <= spp // 2:
                assert not ps.depth()[m].any(), f"{name}: sample spp / 2 has not run after {k}"
        s0 = k
        if k == spp:
            break
    return s0


def sentinel_array(dtype, shape):
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    return np.frombuffer(bytes([SENTINEL]) * n, dtype).reshape(shape).copy()


def check_final(ps, want, what, m=None):
    """The last pass's image and depth against a render's (rgba, depth, counters), and the counters.  An
    IOW-03 pass writes the depth 0 at the pixels m of its rectangle (default: every pixel)."""
    rgba, depth, ctr = want
    same(ps.rgba(), rgba, what + ": final rgba")
    if is_iow(ps.sc):
        depth = sentinel_array(np.float32, depth.shape)
        depth[slice(None) if m is None else m] = 0.0
    same(ps.depth(), depth, what + ": final depth")
    got = ps.counters()
    for k in counter_slots(ps.sc):
        assert int(got[k]) == int(ctr[k]), (what, k)
    if is_iow(ps.sc):
        assert int(got[3]) == 0


# ------------------------------------------------------------- 1-3: final frame, intermediates, counters
@pytest.mark.parametrize("cuts", CUTS, ids=lambda c: "-".join(map(str, c)) if len(c) < 6 else "every")
@pytest.mark.parametrize("name", PR.INW)
def test_inw_passes(gpu, name, cuts):
    sc = scene_of(name)
    s = R.dev_scene(sc)
    try:
        want = cached(("render", name), lambda: render_async(s, sc))
        ps = Passes(s, sc)
        assert run_cuts(ps, cuts, P.SPP, name) == P.SPP
        check_final(ps, want, f"{name} {cuts}")
        ref = PR.counters(name, 0, P.SPP)
        assert all(int(ps.counters()[k]) == v for k, v in ref.items())
    finally:
        R.load().rt_dev_scene_free(s)


@pytest.mark.parametrize("cuts", IOW_CUTS, ids=lambda c: "-".join(map(str, c)) if len(c) < 6 else "every")
def test_iow_passes(gpu, cuts):
    sc = scene_of(PR.IOW)
    s = R.dev_scene(sc)
    try:
        ps = Passes(s, sc)
        assert run_cuts(ps, cuts, PI.SPP, PR.IOW) == PI.SPP
        for spec in (1, 0):  # the frames of the sample-parallel pipeline and of k_iow03
            def frame():
                with R.options(iow_spec=spec):
                    t = R.dev_scene(sc)
                try:
                    return render_async(t, sc)
                finally:
                    R.load().rt_dev_scene_free(t)
            check_final(ps, cached(("render", PR.IOW, spec), frame), f"cam_final {cuts}, iow_spec {spec}")
    finally:
        R.load().rt_dev_scene_free(s)


# ------------------------------------------------------------- 4: ragged shapes
ODD = {"inw01": lambda w, h, spp=5: R.make_scene(R.PRESET_INW01_RANDOM, 1234, 600, width=w, height=h, spp=spp,
                                                 max_bounces=8),
       "iow03": lambda w, h, spp=5: R.make_scene(R.PRESET_IOW03_FINAL, 20250131, 0, width=w, height=h, spp=spp,
                                                 max_bounces=6)}
RECT = dict(tile_x0=5, tile_y0=3, tile_w=20, tile_h=11)
SHAPES = {"37x23": (37, 23, {}), "23x37": (23, 37, {}), "rect": (37, 23, RECT)}


def inside(w, h, rect):
    m = np.zeros((h, w), bool)
    if rect:
        m[rect["tile_y0"]:rect["tile_y0"] + rect["tile_h"], rect["tile_x0"]:rect["tile_x0"] + rect["tile_w"]] = True
    else:
        m[:] = True
    return m.reshape(-1)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("family", list(ODD))
def test_ragged_shapes(gpu, family, shape):
    """Frames whose sides are no multiple of 8, and a rectangle inside one: against the GPU render of the
    same handle and, through the blocking form, against the CPU oracle; outside the rectangle the state
    and the images keep their SENTINEL bytes."""
    from oracle import oracle as O
    w, h, rect = SHAPES[shape]
    sc = ODD[family](w, h)
    p = params_of(sc, **rect)
    m = inside(w, h, rect)
    s = R.dev_scene(sc)
    try:
        want = render_async(s, sc, p)
        ps = Passes(s, sc, p)
        assert ps.run(0, 2) == R.RT_OK
        mid = ps.state().copy()
        assert ps.run(2, 3) == R.RT_OK
        check_final(ps, want, f"{family} {shape}", m)
        st = ps.state()
    finally:
        R.load().rt_dev_scene_free(s)
    for a in (mid, st, ps.rgba(), ps.depth()):
        assert np.all(a[~m].view(np.uint8) == SENTINEL)
        assert not np.all(a[m].view(np.uint8).reshape(m.sum(), -1) == SENTINEL, axis=1).any()
    assert not np.array_equal(mid["acc"][m], st["acc"][m])
    # the blocking form from SENTINEL host buffers, against the oracle's frame
    orgba, odepth, ost = O.render(sc, p)
    n = w * h
    sent = sentinel_array
    res = R.render_passes(sc, (2, 5), want_state=True, params=p, rgba=sent(np.float32, (2, h, w, 4)),
                          depth=None if family == "iow03" else sent(np.float32, (2, h, w)),
                          state=sent(R.PASS_STATE_DTYPE, (h, w)))
    last = res["rgba"][1].reshape(n, 4)
    same(last[m], orgba.reshape(n, 4)[m], f"{family} {shape}: the blocking form against the oracle")
    same(last, want[0], f"{family} {shape}: the blocking form against the GPU render")
    same(res["state"].reshape(-1), st, f"{family} {shape}: the blocking form's state")
    first = res["rgba"][0].reshape(n, 4)
    assert np.all(first[~m].view(np.uint8) == SENTINEL) and not np.array_equal(first[m], last[m])
    same(first[m][:, :3], (mid["acc"][m] * (np.float32(1.0) / np.float32(2))).astype(np.float32),
         f"{family} {shape}: the blocking form's first image")
    if family != "iow03":
        same(res["depth"][1].reshape(n)[m], odepth.reshape(n)[m], f"{family} {shape}: depth against the oracle")
        assert np.all(np.ascontiguousarray(res["depth"].reshape(2, n)[:, ~m]).view(np.uint8) == SENTINEL)
    for k in ("segments", "shadow_queries", "stack_drops", "nan_drops"):
        assert res["stats"][k] == ost[k], k


# ------------------------------------------------------------- 5, 6: many samples, lane refill
@pytest.mark.parametrize("family", list(ODD))
def test_many_samples(gpu, family):
    """70 spp on 9 x 5 pixels: cuts (64, 70), and one pass of 1000 samples, which is clipped at 70."""
    sc = ODD[family](9, 5, 70)
    s = R.dev_scene(sc)
    try:
        want = render_async(s, sc)
        ps = Passes(s, sc)
        assert run_cuts(ps, (64, 70), 70) == 70
        check_final(ps, want, f"{family} (64, 70)")
        one = Passes(s, sc)
        assert one.run(0, 1000) == R.RT_OK
        check_final(one, want, f"{family} one clipped pass")
        same_state(one.state(), ps.state(), family == "iow03", f"{family}: one pass against two")
    finally:
        R.load().rt_dev_scene_free(s)


@pytest.mark.parametrize("family", list(ODD))
def test_lane_refill(gpu, family):
    """One 256-lane block serves the 851 pixels of the 37 x 23 frame: every lane takes several pixels (IOW-03)
    or paths (INW, where the cap holds the path kernel's grid during a pass)."""
    sc = ODD[family](37, 23)
    lib = R.load()
    s = R.dev_scene(sc)
    prev = lib.rt_debug_pass_max_blocks(1)
    try:
        ps = Passes(s, sc)
        assert run_cuts(ps, (2, 5), 5) == 5
    finally:
        assert lib.rt_debug_pass_max_blocks(prev) == 1
    try:
        full = Passes(s, sc)
        assert run_cuts(full, (2, 5), 5) == 5
        check_final(ps, render_async(s, sc), f"{family}: one block")
        same_state(ps.state(), full.state(), family == "iow03", f"{family}: one block against the resident grid")
        assert np.array_equal(ps.counters()[list(counter_slots(sc))], full.counters()[list(counter_slots(sc))])
    finally:
        lib.rt_dev_scene_free(s)


# ------------------------------------------------------------- 7: options
@pytest.mark.parametrize("option,value", [("inw_wide_walk", 0), ("inw_stackless", 0), ("iow_linear", 1),
                                          ("iow_lds_bvh", 0)])
def test_options_do_not_change_results(gpu, option, value):
    name = PR.IOW if option.startswith("iow") else "cam_random600"
    sc = scene_of(name)
    spp = PR.spp_of(name)
    # the linear loop tests every object for every ray: an 8 x 4 rectangle of the frame keeps it short
    rect = dict(tile_x0=4, tile_y0=2, tile_w=8, tile_h=4) if option == "iow_linear" else {}
    m = inside(W, H, rect)
    with R.options(**{option: value}):
        s = R.dev_scene(sc)  # a scene keeps the options it was created with
    try:
        ps = Passes(s, sc, params_of(sc, **rect))
        assert run_cuts(ps, (3, spp // 2, spp), spp, name, m) == spp
        ref = PR.counters(name, 0, spp, m)
        assert all(int(ps.counters()[k]) == v for k, v in ref.items())
        assert np.all(ps.state()[~m].view(np.uint8) == SENTINEL)
    finally:
        R.load().rt_dev_scene_free(s)


# ------------------------------------------------------------- 8: other scenes
def test_textured_inw04_scene(gpu):
    from oracle import oracle as O
    sc = R.make_scene(R.PRESET_INW04_REFSET, 0, 0, width=37, height=23, spp=4)
    for i, t in enumerate([1, 2, 3, 0, 2]):
        sc.geom[i % sc.n, 27] = float(t)
    rng = np.random.default_rng(0)
    sc.textures = [O.noise_texture(600, 100, 2, freq=0.02, lac=2.5, octaves=5),
                   rng.integers(0, 256, (17, 103, 4)).astype(np.uint8),
                   O.noise_texture(600, 100, 0, gradient=[(1, 0.2, 0.1), (0.1, 0.3, 1)], freq=0.05)]
    s = R.dev_scene(sc)
    try:
        want = render_async(s, sc)
        ps = Passes(s, sc)
        assert run_cuts(ps, (1, 2, 4), 4) == 4
        check_final(ps, want, "textured INW-04")
        assert want[2][3] > 0  # shadow queries were counted
    finally:
        R.load().rt_dev_scene_free(s)
    orgba, odepth, _ = O.render(sc)
    same(want[0], orgba.reshape(-1, 4), "textured INW-04: the render against the oracle")


def glass_scene(name):
    """The glass600 / glass600_b fixture's objects as a Scene seen from the side of their slab."""
    f = P.load_fixture(name)
    cam = R.RtCamera()
    cam.pos[:] = (0.0, 4.0, 30.0)
    d = np.array([0.0, -0.1, -1.0])
    cam.dir[:] = [float(v) for v in (d / np.linalg.norm(d)).astype(np.float32)]
    cam.fov_y_rad, cam.aperture, cam.focus_dist = 0.8, 0.1, 25.0
    p = R.RtParams(width=W, height=H, spp=f.spp, max_bounces=f.max_bounces, device=-1)
    return R.Scene(stage=R.RT_STAGE_INW01, desc=None, n=f.n, camera=cam, params=p, geom=f.geom, aabbs=f.aabbs,
                   nodes=f.nodes)


def updated_against_fresh(a, b, update, cuts, what):
    lib = R.load()
    spp = b.params.spp
    s = R.dev_scene(b)
    try:
        fresh = Passes(s, b)
        assert run_cuts(fresh, cuts, spp) == spp
        check_final(fresh, render_async(s, b), what + ": fresh")
    finally:
        lib.rt_dev_scene_free(s)
    s = R.dev_scene(a)
    try:
        before = Passes(s, a)
        assert run_cuts(before, cuts, spp) == spp
        update(s)
        ps = Passes(s, b)
        assert run_cuts(ps, cuts, spp) == spp
    finally:
        lib.rt_dev_scene_free(s)
    assert not np.array_equal(before.rgba(), ps.rgba())  # the update changed the frame
    same(ps.rgba(), fresh.rgba(), what + ": rgba")
    same(ps.depth(), fresh.depth(), what + ": depth")
    same(ps.state(), fresh.state(), what + ": state")
    slots = list(counter_slots(b))
    assert np.array_equal(ps.counters()[slots], fresh.counters()[slots])


@pytest.mark.parametrize("device_build", [False, True])
def test_updated_inw_scene(gpu, device_build):
    a, b = glass_scene("glass600"), glass_scene("glass600_b")

    def update(s):
        rc = R.load().rt_dev_scene_inw_update(s, R.fptr(b.geom), b.n, None if device_build else R.fptr(b.nodes),
                                              R.fptr(b.aabbs) if device_build else None, None, 0, None)
        assert rc == R.RT_OK
    updated_against_fresh(a, b, update, (5, 16), "updated INW scene")


def test_updated_iow_scene(gpu):
    a = R.make_scene(R.PRESET_IOW03_FINAL, 20250131, 0, width=W, height=H, spp=6, max_bounces=8)
    rec = a.records.copy()
    i = np.arange(a.n)
    for k in range(3):
        rec[:, k] += (0.05 * ((i + k) % 3 - 1)).astype(np.float32)
    b = dataclasses.replace(a, records=np.ascontiguousarray(rec), desc=None)
    updated_against_fresh(a, b, lambda s: R.update_iow03(s, b.types, b.records), (2, 6), "updated IOW-03 scene")


# ------------------------------------------------------------- 9: null outputs, errors
@pytest.mark.parametrize("name", ["cam_random600", PR.IOW])
def test_null_outputs(gpu, name):
    sc = scene_of(name)
    spp = PR.spp_of(name)
    s = R.dev_scene(sc)
    try:
        ps = Passes(s, sc, rgba=False, depth=False, counters=False)  # only the state is written
        assert ps.run(0, 3) == R.RT_OK and ps.run(3, spp) == R.RT_OK
        same_state(ps.state(), PR.state(name, spp), name == PR.IOW, f"{name}: state alone")
        img = Passes(s, sc, depth=False)  # an image without a depth
        assert img.run(0, spp) == R.RT_OK
        same(img.rgba(), PR.image(PR.state(name, spp), spp)[0], f"{name}: image without depth")
    finally:
        R.load().rt_dev_scene_free(s)


def test_errors_on_a_device(gpu):
    sc = scene_of("cam_random600")
    s = R.dev_scene(sc)
    try:
        ps = Passes(s, sc)

        def untouched(rc, want):
            assert rc == want
            for t in (ps.d_state, ps.d_rgba, ps.d_depth):
                assert bool((t == SENTINEL).all())
            assert not ps.counters().any()

        untouched(ps.run(0, 4, params_of(sc, spp=8)), R.RT_E_ARG)            # not the scene's spp
        untouched(ps.run(P.SPP, 1), R.RT_E_ARG)                              # s0 >= spp
        untouched(ps.run(0xFFFFFFFF, 2), R.RT_E_ARG)
        untouched(ps.run(0, 4, params_of(sc, width=0)), R.RT_E_ARG)
        untouched(ps.run(0, 4, params_of(sc, show_normal=1)), R.RT_E_UNSUPPORTED)
        untouched(ps.run(P.SPP, 1, params_of(sc, show_normal=1)), R.RT_E_ARG)  # argument errors come first
        untouched(ps.run(3, 0), R.RT_OK)                                      # nothing launched
        rc = R.load().rt_render_pass_async(s, C.byref(sc.camera), C.byref(sc.params), 0, 4, None, ps.d_rgba.data_ptr(),
                                           None, None, None)
        untouched(rc, R.RT_E_ARG)                                             # null state
        assert run_cuts(ps, (8, 16), P.SPP, "cam_random600") == P.SPP         # and the scene still renders
    finally:
        R.load().rt_dev_scene_free(s)


# ------------------------------------------------------------- 10: graph capture
@pytest.mark.parametrize("name", ["cam_random600", PR.IOW])
def test_graph_capture(gpu, name):
    """Three passes captured in one graph (memsets and kernels on one stream: a single branch), replayed
    twice: the eager bytes both times, the counters added twice."""
    sc = scene_of(name)
    spp = PR.spp_of(name)
    cuts = (3, spp // 2, spp)
    s = R.dev_scene(sc)
    try:
        ps = Passes(s, sc)

        def calls():
            s0 = 0
            for c in cuts:
                assert ps.call(s0, c - s0) == R.RT_OK
                s0 = c

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):  # once outside the capture (the occupancy query runs here)
            calls()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        want_state, want_rgba, want_depth, want_ctr = ps.state().copy(), ps.rgba().copy(), ps.depth().copy(), \
            ps.counters().copy()
        same_state(want_state, PR.state(name, spp), name == PR.IOW, f"{name}: eager")
        ps.d_ctr.zero_()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            calls()
        for k in (1, 2):
            for t in (ps.d_state, ps.d_rgba, ps.d_depth):
                t.fill_(SENTINEL)
            graph.replay()
            torch.cuda.synchronize()
            same(ps.state(), want_state, f"replay {k} state")
            same(ps.rgba(), want_rgba, f"replay {k} rgba")
            same(ps.depth(), want_depth, f"replay {k} depth")
            for c in counter_slots(sc):
                assert int(ps.counters()[c]) == k * int(want_ctr[c]), (k, c)
        del graph
    finally:
        torch.cuda.synchronize()
        R.load().rt_dev_scene_free(s)


# ------------------------------------------------------------- 11: resources
# DESIGN.md 5.13's table: which -> (VGPRs, static LDS bytes, resident 256-lane blocks per CU)
RESOURCES = {0: (32, 0, 8), 1: (29, 0, 8), 2: (143, 71936, 2), 3: (147, 53248, 3)}


def test_kernel_resources(gpu):
    """The kernels as loaded: no scratch, and the registers, LDS and occupancy of DESIGN.md 5.13's table."""
    infos = {which: R.pass_kernel_info(which) for which in RESOURCES}
    for which, info in infos.items():
        print(R.PASS_KERNELS[which], info)
    for which, (vgprs, lds, blocks) in RESOURCES.items():
        info = infos[which]
        assert info["scratch_bytes"] == 0, which
        assert (info["vgprs"], info["lds_bytes"], info["blocks_per_cu"]) == (vgprs, lds, blocks), which
