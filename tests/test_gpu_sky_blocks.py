"""Sky blocks (rt_options.inw_sky_blocks): 8x8 pixel blocks whose beam lists are empty
and complete are rendered by k_inw_sky and left out of k_inw_pm's claims.  Every frame here is
compared bit for bit -- colour, depth and the ray-level counters -- with the CPU oracle, and colour,
depth and the segment count with the same frame rendered with inw_sky_blocks = 0;
rt_debug_sky_blocks says how many blocks took the path, so no case passes with the path dead.

The oracle walks the reference's LBVH (it counts the root even for a ray that misses it), the wide
walk and the beam lists their own structures: node visits and primitive tests are each build's own
(tests/test_gpu_parity.py), so against the oracle the four ray-level counters are compared.  On an
all-sky frame neither arm walks or tests anything, and there all six counters agree between the arms."""
import ctypes as C

import pytest

import rt_amd as R
from cases import _scene_cam, compare
from oracle import oracle as O

pytestmark = pytest.mark.gpu

RAY_COUNTERS = ("segments", "shadow_queries", "stack_drops", "nan_drops")
ALL_COUNTERS = ("segments", "node_visits", "prim_tests", "shadow_queries", "stack_drops", "nan_drops")
UP = {"pitch_deg": 55.0}  # from (-60, 15, -60) above the 10-high slab: no ray comes down to it


def _c3(n, cam_over=None, **over):
    """The bench frame's scene and camera (INW-01 random spheres), reduced."""
    return _scene_cam(R.PRESET_INW01_RANDOM, 1234, n, cam_over or {}, **over)


def _render(sc, sky, **opts):
    with R.options(inw_sky_blocks=sky, **opts):
        g, gd, st = R.render(sc)
        return g, gd, st, R.debug_sky_blocks(None)


def _same(a, b):
    return compare(a, b)["exact_frac"] == 1.0


def _check(sc, ref=None, arms=("segments",), **opts):
    """Render with the path on and off: colour, depth and the ray-level counters exact against the
    oracle, colour, depth and the `arms` counters equal between the two.  Returns the on arm's
    (flagged, rendered, blocks)."""
    o, od, ost = ref or O.render(sc)
    g, gd, gst, sky = _render(sc, 1, **opts)
    h, hd, hst, off = _render(sc, 0, **opts)
    print("sky blocks", sky, "off", off, {k: gst[k] for k in ALL_COUNTERS})
    assert off[:2] == (0, 0)
    assert _same(g, o) and _same(gd, od)
    for k in RAY_COUNTERS:
        assert gst[k] == ost[k], (k, gst[k], ost[k])
    assert _same(g, h) and _same(gd, hd)
    for k in arms:
        assert gst[k] == hst[k], (k, gst[k], hst[k])
    p = sc.params
    assert sky[2] == ((p.width + 7) // 8) * ((p.height + 7) // 8)
    return sky


def test_all_sky(gpu):
    sc = _c3(300, UP, width=64, height=40, spp=8)
    sky = _check(sc, arms=ALL_COUNTERS)  # nothing walked or tested in either arm: all six agree
    assert sky == (40, 40, 40)


def test_mixed(gpu):
    """The bench camera: sky above the slab's diamond.  spp 37: no multiple of a pass's 8 samples, an
    odd middle sample."""
    sc = _c3(600, width=96, height=54, spp=37)
    flagged, done, blocks = _check(sc)
    assert 0 < flagged < blocks and done == flagged


@pytest.mark.parametrize("w,h,spp,cam", [(9, 5, 130, UP), (9, 5, 130, {}), (37, 23, 130, {}), (37, 23, 1, {})])
def test_ragged_frames_and_sample_counts(gpu, w, h, spp, cam):
    """Padding units in flagged blocks (9 x 5 looking up: both blocks) and in unflagged ones; spp above
    one wave's 64 lanes with a short last pass (130 = 16 * 8 + 2); spp 1, whose middle sample is sample 0."""
    sc = _c3(600, cam, width=w, height=h, spp=spp)
    flagged, done, blocks = _check(sc)
    if cam:
        assert flagged == done == blocks == 2
    if (w, h) == (37, 23):
        assert 0 < flagged < blocks and done == flagged


def test_tiles(gpu):
    """rt_render_tiles_async, every other 16 x 16 tile of a 100 x 60 frame: the tiles' pixels equal the
    oracle's frame, with the path on and off, and the segment counts agree."""
    import torch

    sc = _c3(600, width=100, height=60, spp=12)
    o, od, _ = O.render(sc)
    lib = R.load()
    ts = 16
    tiles = [(tx, ty) for ty in range((60 + ts - 1) // ts) for tx in range((100 + ts - 1) // ts)][::2]
    dev = torch.device("cuda")
    d_tiles = torch.tensor(tiles, dtype=torch.int32, device=dev).contiguous()
    s = lib.rt_dev_scene_inw(R.fptr(sc.geom), sc.n, 1, R.fptr(sc.nodes), None, 0, sc.params.spp, -1)
    assert s
    seg, sky = {}, {}
    try:
        for on in (1, 0):
            opt = R.default_options()
            opt.inw_sky_blocks = on
            assert lib.rt_dev_scene_set_options(s, C.byref(opt)) == 0
            out = torch.zeros((len(tiles), ts, ts, 4), dtype=torch.float32, device=dev)
            dep = torch.zeros((len(tiles), ts, ts), dtype=torch.float32, device=dev)
            ctr = torch.zeros(6, dtype=torch.int64, device=dev)
            assert lib.rt_render_tiles_async(s, C.byref(sc.camera), C.byref(sc.params), d_tiles.data_ptr(), len(tiles),
                                             ts, out.data_ptr(), dep.data_ptr(), ctr.data_ptr(),
                                             torch.cuda.current_stream().cuda_stream) == 0
            torch.cuda.synchronize()
            sky[on] = R.debug_sky_blocks(s)
            seg[on] = int(ctr[0].item())
            a, d = out.cpu().numpy(), dep.cpu().numpy()
            for i, (tx, ty) in enumerate(tiles):
                hh, ww = min(ts, 60 - ty * ts), min(ts, 100 - tx * ts)
                assert _same(a[i, :hh, :ww], o[ty * ts:ty * ts + hh, tx * ts:tx * ts + ww]), (on, tx, ty)
                assert _same(d[i, :hh, :ww], od[ty * ts:ty * ts + hh, tx * ts:tx * ts + ww]), (on, tx, ty)
                assert not a[i, hh:].any() and not a[i, :, ww:].any() and not d[i, hh:].any()  # the tiles' padding
    finally:
        lib.rt_dev_scene_free(s)
    print("tiles: sky blocks", sky, "segments", seg)
    assert seg[1] == seg[0]
    assert sky[0][:2] == (0, 0) and sky[1][2] == len(tiles) * 4
    assert 0 < sky[1][0] < sky[1][2] and sky[1][1] == sky[1][0]


def test_not_eligible_lights(gpu):
    sc = R.make_scene(R.PRESET_INW04_CORNELL, 7, 0, width=32, height=24, spp=4)
    assert _check(sc)[:2] == (0, 0)


def test_not_eligible_multifocus(gpu):
    sc = _c3(300, width=40, height=24, spp=6)
    focus = [6.0, 14.0]
    o, od, ost = O.render_inw_mf(sc, focus)
    with R.options(inw_sky_blocks=1):
        g, gd, gst = R.render_inw_mf(sc, focus)
        sky = R.debug_sky_blocks(None)
    assert sky == (0, 0, 15)
    assert _same(g, o) and _same(gd, od)
    for k in RAY_COUNTERS:
        assert gst[k] == ost[k], k


@pytest.mark.parametrize("opts", [{"inw_beams": 0}, {"inw_order": 2}])
def test_not_eligible_options(gpu, opts):
    """No beam lists; a forced sample-major frame."""
    sc = _c3(300, width=40, height=24, spp=6)
    assert _check(sc, **opts)[:2] == (0, 0)


def test_not_eligible_pixel_rays(gpu):
    """rt_debug_pixel_rays counts every segment at its pixel, k_inw_pm's job: no sky blocks while it is set."""
    import torch

    sc = _c3(300, width=40, height=24, spp=6)
    o, od, ost = O.render(sc)
    lib = R.load()
    buf = torch.zeros(40 * 24, dtype=torch.int32, device="cuda")
    assert lib.rt_debug_pixel_rays(buf.data_ptr()) == 0
    try:
        g, gd, gst, sky = _render(sc, 1)
        torch.cuda.synchronize()
    finally:
        lib.rt_debug_pixel_rays(None)
    assert sky == (0, 0, 15)
    assert _same(g, o) and _same(gd, od) and gst["segments"] == ost["segments"]
    assert int(buf.sum().item()) == ost["segments"]


def test_abort_on_a_zero_direction_component(gpu):
    """Looking along +x but for a yaw of 1e-6 degrees, with a pinhole lens: the centre column's pixel
    directions have z of about 1.5e-8, so their beam lists are built (at z == 0 exactly k_inw_beam
    turns them off and the block is never flagged), but in the camera ray both -60 + 40 z and
    -60 + z round to -60 and the ray's d.z is 0.  Such rays fail the beam lists' test: the flagged
    blocks that hold them go back to k_inw_pm (rendered < flagged) and the frame stays exact."""
    sc = _c3(600, {"pitch_deg": 0.0, "yaw_deg": 1e-6, "aperture": 0.0}, width=64, height=48, spp=9)
    flagged, done, blocks = _check(sc)
    assert 0 < done < flagged <= blocks
