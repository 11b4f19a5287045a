"""Progressive sample passes over packed tile lists (rt_render_pass_tiles_async) on the GPU.  Every equality
is a byte equality.  A slot inside the image is its pixel under rt_render_pass_async: every intermediate
state and image against tests/pass_ref.py (the fixture frames) or against rt_render_pass_async of the same
handle (the ragged frame), through the slot mapping of tests/pass_tiles_ref.py.  A slot outside the image
keeps its state bytes and gets the zero image.  The last pass's packed image is rt_render_tiles_async's for
the same list, slots outside the image included; so is the depth on INW scenes (an IOW-03 pass writes the
depth 0, which the IOW-03 renders leave unwritten)."""
import ctypes as C

import numpy as np
import pytest

import pass_ref as PR
import pass_tiles_ref as PT
import path_iow_ref as PI
import path_ref as P
import rt_amd as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = 0xCD
INW_COUNTERS = (0, 3, 4, 5)  # segments, shadow queries, dropped pushes, NaN directions: the reference's
IOW_COUNTERS = (0, 4, 5)
W, H = PR.W, PR.H

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


def filled(nbytes):
    return torch.full((max(nbytes, 16),), SENTINEL, dtype=torch.uint8, device=torch.device("cuda"))


def stream():
    return torch.cuda.current_stream().cuda_stream


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


class TilePasses:
    """The packed buffers of one list's passes, all SENTINEL bytes at first, and the list's counters."""

    def __init__(self, s, sc, tiles, T):
        self.s, self.sc, self.T = s, sc, T
        self.tiles = np.ascontiguousarray(tiles, np.int32).reshape(-1, 2)
        self.n_tiles = len(self.tiles)
        self.n = self.n_tiles * T * T
        self.pixel, self.inside = PT.slots(self.tiles, T, sc.params.width, sc.params.height)
        dev = torch.device("cuda")
        self.d_tiles = torch.from_numpy(self.tiles.copy()).to(dev)
        self.d_state, self.d_rgba, self.d_depth = filled(self.n * 32), filled(self.n * 16), filled(self.n * 4)
        self.d_ctr = torch.zeros(6, dtype=torch.int64, device=dev)

    def run(self, s0, ns, params=None):
        rc = R.render_pass_tiles(self.s, self.sc.camera, params or self.sc.params, self.d_tiles, self.n_tiles, self.T,
                                 s0, ns, self.d_state, self.d_rgba, self.d_depth, self.d_ctr, stream())
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

    def check(self, want_state, want_rgba, want_depth, what):
        """The slots inside the image against per-pixel references ((W * H,) arrays); outside, the state's
        SENTINEL bytes and the zero image."""
        m, px = self.inside, self.pixel[self.inside]
        st, rgba, depth = self.state(), self.rgba(), self.depth()
        same_state(st[m], want_state[px], is_iow(self.sc), what + ": state")
        same(rgba[m], want_rgba[px], what + ": image")
        same(depth[m], want_depth[px], what + ": depth")
        assert np.all(st[~m].view(np.uint8) == SENTINEL), what + ": a state outside the image was written"
        assert not rgba[~m].view(np.uint32).any() and not depth[~m].view(np.uint32).any(), what + ": outside is not zero"

    def check_final(self, what):
        """The last pass against rt_render_tiles_async of the same handle and list."""
        d_rgba, d_depth = filled(self.n * 16), filled(self.n * 4)
        d_ctr = torch.zeros(6, dtype=torch.int64, device=d_rgba.device)
        rc = R.load().rt_render_tiles_async(self.s, C.byref(self.sc.camera), C.byref(self.sc.params),
                                            self.d_tiles.data_ptr(), self.n_tiles, self.T, d_rgba.data_ptr(),
                                            d_depth.data_ptr(), d_ctr.data_ptr(), stream())
        torch.cuda.synchronize()
        assert rc == R.RT_OK
        same(self.rgba(), d_rgba.cpu().numpy()[: self.n * 16].view(np.float32).reshape(self.n, 4), what + ": final rgba")
        if is_iow(self.sc):
            assert not self.depth().view(np.uint32).any(), what + ": an IOW-03 pass writes the depth 0"
        else:
            same(self.depth(), d_depth.cpu().numpy()[: self.n * 4].view(np.float32), what + ": final depth")
        ctr = d_ctr.cpu().numpy()
        for k in counter_slots(self.sc):
            assert int(self.counters()[k]) == int(ctr[k]), (what, k)


# ------------------------------------------------------------- the fixture frames: one tile, rows 9..15 outside
CUTS = {"one": lambda spp: (spp,), "three": lambda spp: (3, spp // 2, spp), "every": lambda spp: tuple(range(1, spp + 1))}


@pytest.mark.parametrize("cuts", list(CUTS))
@pytest.mark.parametrize("name", PR.INW + [PR.IOW])
def test_fixture_frames(gpu, name, cuts):
    sc = scene_of(name)
    spp = PR.spp_of(name)
    s = R.dev_scene(sc)
    try:
        ps = TilePasses(s, sc, [(0, 0)], 16)
        assert ps.inside.sum() == W * H and (~ps.inside).sum() == 16 * 7
        s0 = 0
        for k in CUTS[cuts](spp):
            assert ps.run(s0, k - s0) == R.RT_OK, (s0, k)
            want = PR.state(name, k)
            rgba, depth = PR.image(want, k)
            ps.check(want, rgba, depth, f"{name}: after {k} samples")
            s0 = k
        ps.check_final(f"{name} {cuts}")
        ref = PR.counters(name, 0, spp)
        assert all(int(ps.counters()[k]) == v for k, v in ref.items())
    finally:
        R.load().rt_dev_scene_free(s)


# ------------------------------------------------------------- the ragged frame
ODD = {"inw01": lambda w, h, spp=5: R.make_scene(R.PRESET_INW01_RANDOM, 1234, 600, width=w, height=h, spp=spp,
                                                 max_bounces=8),
       "iow03": lambda w, h, spp=5: R.make_scene(R.PRESET_IOW03_FINAL, 20250131, 0, width=w, height=h, spp=spp,
                                                 max_bounces=6)}
RW, RH = 37, 23
PASSES = ((0, 2), (2, 3))


def rect_reference(s, sc):
    """rt_render_pass_async's states and images of the whole frame after each of PASSES, and the counters."""
    n = RW * RH
    d_state, d_rgba, d_depth = filled(n * 32), filled(n * 16), filled(n * 4)
    d_ctr = torch.zeros(6, dtype=torch.int64, device=d_state.device)
    out = []
    for s0, ns in PASSES:
        rc = R.load().rt_render_pass_async(s, C.byref(sc.camera), C.byref(sc.params), s0, ns, d_state.data_ptr(),
                                           d_rgba.data_ptr(), d_depth.data_ptr(), d_ctr.data_ptr(), stream())
        torch.cuda.synchronize()
        assert rc == R.RT_OK
        out.append((d_state.cpu().numpy()[: n * 32].view(R.PASS_STATE_DTYPE).copy(),
                    d_rgba.cpu().numpy()[: n * 16].view(np.float32).reshape(n, 4).copy(),
                    d_depth.cpu().numpy()[: n * 4].view(np.float32).copy()))
    return out, d_ctr.cpu().numpy()


def run_list(s, sc, ref, tiles, T, what):
    ps = TilePasses(s, sc, tiles, T)
    for (s0, ns), (st, rgba, depth) in zip(PASSES, ref):
        assert ps.run(s0, ns) == R.RT_OK
        ps.check(st, rgba, depth, f"{what}: after {s0 + ns} samples")
    ps.check_final(what)
    return ps


def ragged_lists():
    deal = R.tile_deal(RW, RH, 16, 3)
    assert len(deal) == 6
    return {"full16": (deal, 16), "share1of3": (PT.shares(deal, 3)[1], 16), "two16": ([(2, 1), (0, 0)], 16),
            "full32": (R.tile_deal(RW, RH, 32, 1), 32)}


@pytest.mark.parametrize("which", ["full16", "share1of3", "two16", "full32"])
@pytest.mark.parametrize("family", list(ODD))
def test_ragged_frame(gpu, family, which):
    sc = ODD[family](RW, RH)
    tiles, T = ragged_lists()[which]
    s = R.dev_scene(sc)
    try:
        ref, _ = cached(("rect", family), lambda: rect_reference(s, sc))
        ps = run_list(s, sc, ref, tiles, T, f"{family} {which}")
        assert (~ps.inside).any()  # every list has slots outside the image
    finally:
        R.load().rt_dev_scene_free(s)


@pytest.mark.parametrize("family", list(ODD))
def test_partition_counters(gpu, family):
    """The counters summed over the three shares of a 3-device deal are the whole frame's passes'."""
    sc = ODD[family](RW, RH)
    s = R.dev_scene(sc)
    try:
        ref, ctr = cached(("rect", family), lambda: rect_reference(s, sc))
        total = np.zeros(6, np.int64)
        for r, share in enumerate(PT.shares(R.tile_deal(RW, RH, 16, 3), 3)):
            total += run_list(s, sc, ref, share, 16, f"{family} share {r}").counters()
        for k in counter_slots(sc):
            assert int(total[k]) == int(ctr[k]), k
    finally:
        R.load().rt_dev_scene_free(s)


# ------------------------------------------------------------- lane refill, options, resources
@pytest.mark.parametrize("family", list(ODD))
def test_one_block_refills_across_tiles(gpu, family):
    """One 256-lane block serves the six tiles of the 37 x 23 frame."""
    sc = ODD[family](RW, RH)
    lib = R.load()
    s = R.dev_scene(sc)
    try:
        ref, ctr = cached(("rect", family), lambda: rect_reference(s, sc))
        prev = lib.rt_debug_pass_max_blocks(1)
        try:
            ps = run_list(s, sc, ref, R.tile_deal(RW, RH, 16, 3), 16, f"{family}: one block")
        finally:
            assert lib.rt_debug_pass_max_blocks(prev) == 1
        for k in counter_slots(sc):
            assert int(ps.counters()[k]) == int(ctr[k]), k
    finally:
        lib.rt_dev_scene_free(s)


@pytest.mark.parametrize("family,option,value,tiles", [("inw01", "inw_wide_walk", 0, None),
                                                        ("iow03", "iow_linear", 1, [(2, 1)])])
def test_options_do_not_change_results(gpu, family, option, value, tiles):
    """The reference comes from a scene with the default options.  (The linear loop tests every object for
    every ray: the tile (2, 1), with 35 pixels inside the image, keeps it short.)"""
    sc = ODD[family](RW, RH)
    s = R.dev_scene(sc)
    try:
        ref, _ = cached(("rect", family), lambda: rect_reference(s, sc))
    finally:
        R.load().rt_dev_scene_free(s)
    with R.options(**{option: value}):
        s = R.dev_scene(sc)  # a scene keeps the options it was created with
    try:
        run_list(s, sc, ref, tiles or R.tile_deal(RW, RH, 16, 3), 16, f"{family} {option}={value}")
    finally:
        R.load().rt_dev_scene_free(s)


def test_errors_on_a_device(gpu):
    sc = ODD["inw01"](RW, RH)
    s = R.dev_scene(sc)
    try:
        ps = TilePasses(s, sc, [(0, 0), (2, 1)], 16)

        def untouched(rc, want):
            assert rc == want
            for t in (ps.d_state, ps.d_rgba, ps.d_depth):
                assert bool((t == SENTINEL).all())
            assert not ps.counters().any()

        def params(**kw):
            p = R.RtParams.from_buffer_copy(sc.params)
            for k, v in kw.items():
                setattr(p, k, v)
            return p

        untouched(ps.run(0, 4, params(spp=8)), R.RT_E_ARG)             # not the scene's spp
        untouched(ps.run(5, 1), R.RT_E_ARG)                            # s0 >= spp
        untouched(ps.run(0, 4, params(show_normal=1)), R.RT_E_UNSUPPORTED)
        untouched(ps.run(5, 1, params(show_normal=1)), R.RT_E_ARG)     # argument errors come first
        untouched(ps.run(3, 0), R.RT_OK)                               # nothing launched
        for n, T in ((0, 16), (-1, 16), (2, 8), (2, 24), (2, 0)):
            rc = R.render_pass_tiles(s, sc.camera, sc.params, ps.d_tiles, n, T, 0, 2, ps.d_state, ps.d_rgba, ps.d_depth,
                                     ps.d_ctr, stream())
            torch.cuda.synchronize()
            untouched(rc, R.RT_E_ARG)
        # n_tiles * T * T = 2^31 + 2^10 slots: refused before any of them is touched (the buffers hold two tiles)
        rc = R.render_pass_tiles(s, sc.camera, sc.params, ps.d_tiles, (1 << 21) + 1, 32, 0, 2, ps.d_state, ps.d_rgba,
                                 ps.d_depth, ps.d_ctr, stream())
        torch.cuda.synchronize()
        untouched(rc, R.RT_E_ARG)
        rc = R.render_pass_tiles(s, sc.camera, sc.params, None, 2, 16, 0, 2, ps.d_state, ps.d_rgba, ps.d_depth,
                                 ps.d_ctr, stream())
        untouched(rc, R.RT_E_ARG)                                      # null tiles
        rc = R.render_pass_tiles(s, sc.camera, sc.params, ps.d_tiles, 2, 16, 0, 2, None, ps.d_rgba, ps.d_depth,
                                 ps.d_ctr, stream())
        untouched(rc, R.RT_E_ARG)                                      # null state
        assert ps.run(0, 5) == R.RT_OK                                 # and the scene still renders
        ps.check_final("after the errors")
    finally:
        R.load().rt_dev_scene_free(s)


# DESIGN.md 5.16's table: which -> (VGPRs, static LDS bytes, resident 256-lane blocks per CU)
RESOURCES = {16: (30, 0, 8), 17: (29, 0, 8), 18: (147, 71936, 2), 19: (154, 53248, 3)}


def test_kernel_resources(gpu):
    """The tile-list instances as loaded: no scratch, and the registers, LDS and occupancy of DESIGN.md
    5.16's table."""
    infos = {which: R.pass_kernel_info(which) for which in RESOURCES}
    for which, info in infos.items():
        print(R.PASS_TILE_KERNELS[which], info)
    for which, want in RESOURCES.items():
        info = infos[which]
        assert info["scratch_bytes"] == 0, which
        assert (info["vgprs"], info["lds_bytes"], info["blocks_per_cu"]) == want, which
