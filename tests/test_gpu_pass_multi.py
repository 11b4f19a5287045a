"""Progressive sample passes on a device group (rt_render_pass_multi_async, rt_render_passes_inw_multi) on
the GPU.  A one-device group, as in tests/test_gpu_multi.py: its tiles still travel through RCCL (device 0
sends to itself).  Every equality is a byte equality: each pass's device-0 image and depth against
rt_render_pass_async's for the same cuts, the last against rt_render_multi_async and rt_render_image_async
with the ray-level counters.  Where a second GPU exists the first case also runs on devices [0, 1].  Group
passes are not captured into graphs here: a group works on several streams."""
import ctypes as C

import numpy as np
import pytest

import rt_amd as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = 0xCD
INW_COUNTERS = (0, 3, 4, 5)
IOW_COUNTERS = (0, 4, 5)
CASES = {
    "inw01": (lambda: R.make_scene(R.PRESET_INW01_RANDOM, 1234, 2000, width=100, height=60, spp=12), 16, (4, 12)),
    "cornell": (lambda: R.make_scene(R.PRESET_INW04_CORNELL, 7, 0, width=64, height=48, spp=9), 32, (1, 5, 9)),
    "iow03": (lambda: R.make_scene(R.PRESET_IOW03_FINAL, 20250131, 0, width=37, height=23, spp=5, max_bounces=6), 16,
              (2, 5)),
}


def is_iow(sc):
    return sc.stage == R.RT_STAGE_IOW03


def stream():
    return torch.cuda.current_stream().cuda_stream


def same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero(got.reshape(-1).view(np.uint32) != want.reshape(-1).view(np.uint32))
        raise AssertionError(f"{what}: {len(bad)} of {got.size} words differ, first {bad[0]}")


class Frame:
    """Device-0 image, depth and counters of one frame, SENTINEL bytes at first."""

    def __init__(self, p):
        self.n = p.width * p.height
        dev = torch.device("cuda", 0)
        self.d_rgba = torch.full((self.n * 16,), SENTINEL, dtype=torch.uint8, device=dev)
        self.d_depth = torch.full((self.n * 4,), SENTINEL, dtype=torch.uint8, device=dev)
        self.d_ctr = torch.zeros(6, dtype=torch.int64, device=dev)

    def rgba(self):
        return self.d_rgba.cpu().numpy().view(np.float32).reshape(self.n, 4)

    def depth(self):
        return self.d_depth.cpu().numpy().view(np.float32)

    def counters(self):
        return self.d_ctr.cpu().numpy()

    def ptrs(self, image=True):
        return (self.d_rgba.data_ptr() if image else None, self.d_depth.data_ptr() if image else None,
                self.d_ctr.data_ptr())


class Group:
    """A group on `devices` with the scene replicated on each."""

    def __init__(self, sc, devices=(0,)):
        lib = R.load()
        self.sc, self.devices = sc, devices
        self.handles = [R.dev_scene(sc, device=d) for d in devices]
        self.scenes = (C.c_void_p * len(devices))(*self.handles)
        self.g = lib.rt_group_create((C.c_int * len(devices))(*devices), len(devices))
        assert self.g

    def pass_(self, s0, ns, tile, fr, image=True, params=None):
        rc = R.load().rt_render_pass_multi_async(self.g, self.scenes, C.byref(self.sc.camera),
                                                 C.byref(params or self.sc.params), tile, s0, ns, *fr.ptrs(image), stream())
        torch.cuda.synchronize()
        return rc

    def frame(self, tile, fr, params=None):
        rc = R.load().rt_render_multi_async(self.g, self.scenes, C.byref(self.sc.camera),
                                            C.byref(params or self.sc.params), tile, *fr.ptrs(), stream())
        torch.cuda.synchronize()
        return rc

    def close(self):
        torch.cuda.synchronize()
        R.load().rt_group_free(self.g)
        for h in self.handles:
            R.load().rt_dev_scene_free(h)


def single_device(s, sc, cuts, params=None):
    """rt_render_pass_async's (rgba, depth) after each cut, its counters, and rt_render_image_async's frame."""
    lib = R.load()
    p = params or sc.params
    fr = Frame(p)
    d_state = torch.full((fr.n * 32,), SENTINEL, dtype=torch.uint8, device=fr.d_rgba.device)
    out, s0 = [], 0
    for c in cuts:
        assert lib.rt_render_pass_async(s, C.byref(sc.camera), C.byref(p), s0, c - s0, d_state.data_ptr(), *fr.ptrs(),
                                        stream()) == R.RT_OK
        torch.cuda.synchronize()
        out.append((fr.rgba().copy(), fr.depth().copy()))
        s0 = c
    img = Frame(p)
    assert lib.rt_render_image_async(s, C.byref(sc.camera), C.byref(p), *img.ptrs(), stream()) == R.RT_OK
    torch.cuda.synchronize()
    return out, fr.counters(), img


def run_case(name, devices):
    make, tile, cuts = CASES[name]
    sc = make()
    slots = IOW_COUNTERS if is_iow(sc) else INW_COUNTERS
    grp = Group(sc, devices)
    try:
        want, want_ctr, img = single_device(grp.handles[0], sc, cuts)
        fr = Frame(sc.params)
        s0 = 0
        for c, (rgba, depth) in zip(cuts, want):
            assert grp.pass_(s0, c - s0, tile, fr) == R.RT_OK, (s0, c)
            same(fr.rgba(), rgba, f"{name}: image after {c} samples")
            same(fr.depth(), depth, f"{name}: depth after {c} samples")
            s0 = c
        for k in slots:
            assert int(fr.counters()[k]) == int(want_ctr[k]), k
        # the last pass is the frame of rt_render_multi_async and rt_render_image_async
        whole = Frame(sc.params)
        assert grp.frame(tile, whole) == R.RT_OK
        same(fr.rgba(), whole.rgba(), f"{name}: against rt_render_multi_async")
        same(fr.rgba(), img.rgba(), f"{name}: against rt_render_image_async")
        if not is_iow(sc):  # (the IOW-03 renders leave the depth unwritten; a pass writes 0)
            same(fr.depth(), whole.depth(), f"{name}: depth against rt_render_multi_async")
            same(fr.depth(), img.depth(), f"{name}: depth against rt_render_image_async")
        for k in slots:
            assert int(fr.counters()[k]) == int(whole.counters()[k]) == int(img.counters()[k]), k
        # a pass without an image, then one with it: the two-pass result
        two = Frame(sc.params)
        assert grp.pass_(0, cuts[0], tile, two, image=False) == R.RT_OK
        assert bool((two.d_rgba == SENTINEL).all()) and bool((two.d_depth == SENTINEL).all())
        assert grp.pass_(cuts[0], sc.params.spp, tile, two) == R.RT_OK  # clipped at spp
        same(two.rgba(), fr.rgba(), f"{name}: after a pass without an image")
        same(two.depth(), fr.depth(), f"{name}: depth after a pass without an image")
        for k in slots:
            assert int(two.counters()[k]) == int(fr.counters()[k]), k
    finally:
        grp.close()


@pytest.mark.parametrize("name", list(CASES))
def test_one_device_group(gpu, name):
    run_case(name, (0,))


def test_two_device_group(gpu):
    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU: no group of more than one device")
    run_case("inw01", (0, 1))


def test_sample_tracking_and_state_ownership(gpu):
    make, tile, _ = CASES["inw01"]
    sc = make()
    spp = sc.params.spp
    small = R.RtParams.from_buffer_copy(sc.params)
    small.width, small.height = 64, 40
    grp = Group(sc)
    try:
        want, _, _ = single_device(grp.handles[0], sc, (4, spp))
        want_small, _, _ = single_device(grp.handles[0], sc, (4, spp), small)
        fr = Frame(sc.params)
        assert grp.pass_(4, 8, tile, fr) == R.RT_E_ARG               # no frame begun: the count is 0
        assert grp.pass_(spp, 1, tile, fr) == R.RT_E_ARG             # s0 >= spp
        assert bool((fr.d_rgba == SENTINEL).all()) and not fr.counters().any()
        assert grp.pass_(0, 4, tile, fr) == R.RT_OK
        same(fr.rgba(), want[0][0], "first pass")
        for bad in (3, 5):
            assert grp.pass_(bad, 2, tile, fr) == R.RT_E_ARG, bad    # neither 0 nor the count
        same(fr.rgba(), want[0][0], "a refused pass wrote nothing")
        # a call a scene would refuse is refused before the group is touched: the frame's progress stays
        other = R.RtParams.from_buffer_copy(sc.params)
        other.spp = spp + 4
        assert grp.pass_(4, 2, tile, fr, params=other) == R.RT_E_ARG          # not the scenes' spp
        assert grp.pass_(0, 2, tile, fr, params=other) == R.RT_E_ARG
        other.spp, other.max_bounces = spp, -1
        assert grp.pass_(4, 2, tile, fr, params=other) == R.RT_E_ARG          # bad params
        other.max_bounces, other.show_normal = sc.params.max_bounces, 1
        assert grp.pass_(4, 2, tile, fr, params=other) == R.RT_E_UNSUPPORTED
        assert grp.pass_(5, 2, tile, fr, params=other) == R.RT_E_ARG          # argument errors come first
        same(fr.rgba(), want[0][0], "the refused passes wrote nothing")
        # a whole frame between two passes disturbs neither states nor count
        whole = Frame(sc.params)
        assert grp.frame(tile, whole) == R.RT_OK
        assert grp.pass_(4, spp - 4, tile, fr) == R.RT_OK
        same(fr.rgba(), want[1][0], "second pass after a refused one and a whole frame")
        same(fr.depth(), want[1][1], "its depth")
        same(fr.rgba(), whole.rgba(), "the frame")
        # a new frame may begin at any time; another frame size resets the count
        assert grp.pass_(0, 4, tile, fr) == R.RT_OK
        sm = Frame(small)
        assert grp.pass_(4, spp - 4, tile, sm, params=small) == R.RT_E_ARG   # the deal changes: its count is 0
        assert grp.pass_(0, 4, tile, sm, params=small) == R.RT_OK
        same(sm.rgba(), want_small[0][0], "the smaller frame's first pass")
        assert grp.pass_(4, spp - 4, tile, fr) == R.RT_E_ARG                   # ... and the larger frame's is gone
        assert grp.pass_(4, spp - 4, tile, sm, params=small) == R.RT_OK
        same(sm.rgba(), want_small[1][0], "the smaller frame's second pass")
        same(sm.depth(), want_small[1][1], "its depth")
    finally:
        grp.close()


def test_blocking_form(gpu):
    make, tile, cuts = CASES["cornell"]
    sc = make()
    one = R.render_passes(sc, cuts)
    multi = R.render_passes_multi(sc, [0], cuts, tile=tile)
    same(multi["rgba"], one["rgba"], "rt_render_passes_inw_multi against rt_render_passes_inw")
    same(multi["depth"], one["depth"], "depth")
    for k in ("segments", "shadow_queries", "stack_drops", "nan_drops"):
        assert multi["stats"][k] == one["stats"][k], k
    assert one["stats"]["shadow_queries"] > 0
