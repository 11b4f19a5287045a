"""Frames of moving, rotated, unequal-scale ellipsoids and cuboids (tests/cases.py _mixed; what makes
them worth rendering is asserted on the CPU, tests/test_mixed_scenes.py): the general 7-float4 object
records together with time-bin trees, beam lists per bin, sky blocks and the beam prune's box step,
INW-04 shadow queries with a time ratio beside moving lights, updates between sphere scenes and these,
and caller boxes the objects stick out of (such scenes take the reference walk, DESIGN.md §2 "Objects
inside their leaf boxes").  Every comparison is bit for bit: colour, depth, the ray-level counters."""
import ctypes as C

import numpy as np
import pytest

import rt_amd as R
from cases import CASES, MIXED_CASES, SHRUNK_CASES, _mixed01, _mixed04, compare
from oracle import oracle as O

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

RAY_COUNTERS = ("segments", "shadow_queries", "stack_drops", "nan_drops")
_cache = {}


def _case(name):
    """(scene, oracle frame, oracle depth, oracle stats), computed once."""
    if name not in _cache:
        sc = CASES[name]()
        _cache[name] = (sc,) + tuple(O.render(sc))
    return _cache[name]


def _render(sc, over):
    """A blocking render with the default options changed by `over`: colour and depth stacked, stats."""
    with R.options(**{**R.default_options().as_dict(), **over}):
        img, depth, st = R.render(sc)
    return np.concatenate([img, depth[..., None]], axis=2), st


def _default(name):
    key = name + ":gpu"
    if key not in _cache:
        _cache[key] = _render(_case(name)[0], {})
    return _cache[key]


def _assert_same_frames(name, over):
    a, sa = _default(name)
    b, sb = _render(_case(name)[0], over)
    same = (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
    assert same.all(), (over, int((~same.all(axis=2)).sum()), np.argwhere(~same.all(axis=2))[:10].tolist())
    for k in RAY_COUNTERS:
        assert sa[k] == sb[k], (over, k, sa[k], sb[k])


INW01_ARMS = [
    {"inw_time_bins": 0}, {"inw_time_bins": 3}, {"inw_time_bins": 16},
    {"inw_walk_bins": 0}, {"inw_beam_bins": 0},
    {"inw_beams": 0}, {"inw_beams": 2},
    {"inw_beam_prune": 0}, {"inw_beam_prune": 1},
    {"inw_sky_blocks": 0},
    {"inw_order": -1}, {"inw_order": 1}, {"inw_order": 2},
    {"inw_fused_cull": 0}, {"inw_ri_grid": 0}, {"inw_lds_nodes": 0}, {"inw_compact_nodes": 0},
    {"inw_qnodes": 1, "inw_order": 1},
    {"inw_wide_walk": 0},
]
INW04_ARMS = [{"inw_order": 1}, {"inw_order": 2}, {"inw_order": -1}, {"inw_time_bins": 0}, {"inw_time_bins": 4},
              {"inw_beams": 0}, {"inw_wide_walk": 0}]
SHRUNK_ARMS = [{"inw_beams": 0}, {"inw_beam_prune": 0}, {"inw_time_bins": 0}, {"inw_order": -1}]


def _id(over):
    return ",".join(f"{k}={v}" for k, v in over.items())


@pytest.mark.parametrize("over", INW01_ARMS, ids=_id)
def test_inw01_mixed_strategies_bit_identical(gpu, over):
    _assert_same_frames("inw01_mixed_moving", over)


@pytest.mark.parametrize("over", INW04_ARMS, ids=_id)
def test_inw04_mixed_strategies_bit_identical(gpu, over):
    _assert_same_frames("inw04_mixed_moving", over)


@pytest.mark.parametrize("over", SHRUNK_ARMS, ids=_id)
def test_shrunk_boxes_strategies_bit_identical(gpu, over):
    _assert_same_frames("inw01_mixed_shrunk06", over)


@pytest.mark.parametrize("name", MIXED_CASES + SHRUNK_CASES)
def test_default_frame_equals_the_oracle(gpu, name):
    sc, o, od, ost = _case(name)
    g, gst = _default(name)
    c, cd = compare(g[..., 0:4], o), compare(g[..., 4], od)
    bad = (g.view(np.uint32) != np.concatenate([o, od[..., None]], axis=2).view(np.uint32)).any(axis=2)
    print(name, c, cd, "mismatching pixels", int(bad.sum()), np.argwhere(bad)[:5].tolist())
    assert c["nan_mismatch"] == 0 and c["exact_frac"] == 1.0, (c, int(bad.sum()))
    assert cd["exact_frac"] == 1.0, cd
    for k in RAY_COUNTERS:
        assert gst[k] == ost[k], (k, gst[k], ost[k])


class _Dev:
    """A device scene of a packed scene's geometry, rendered with any scene's camera and parameters."""

    def __init__(self, sc):
        self.lib = R.load()
        self.s = self.lib.rt_dev_scene_inw(R.fptr(sc.geom), sc.n, sc.layout, R.fptr(sc.nodes),
                                           R.fptr(sc.lights if sc.n_lights else None), sc.n_lights, sc.params.spp, -1)
        assert self.s

    def update(self, sc, device_build):
        rc = self.lib.rt_dev_scene_inw_update(self.s, R.fptr(sc.geom), sc.n, None if device_build else R.fptr(sc.nodes),
                                              R.fptr(sc.aabbs), R.fptr(sc.lights if sc.n_lights else None), sc.n_lights,
                                              None)
        assert rc == R.RT_OK, rc

    def frame(self, sc):
        """(colour, depth, the six counters, rt_debug_path, rt_debug_sky_blocks) of one frame."""
        p = sc.params
        img = torch.zeros((p.height, p.width, 4), dtype=torch.float32, device="cuda")
        dep = torch.zeros((p.height, p.width), dtype=torch.float32, device="cuda")
        ctr = torch.zeros(6, dtype=torch.int64, device="cuda")
        assert self.lib.rt_render_image_async(self.s, C.byref(sc.camera), C.byref(p), img.data_ptr(), dep.data_ptr(),
                                              ctr.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        return img.cpu().numpy(), dep.cpu().numpy(), ctr.cpu().numpy(), R.debug_path(self.s), R.debug_sky_blocks(self.s)

    def free(self):
        self.lib.rt_dev_scene_free(self.s)


def _ray_counters(ctr):
    return [int(ctr[i]) for i in (0, 3, 4, 5)]  # segments, shadow queries, stack drops, NaN drops


def test_default_inw01_frame_takes_the_paths_it_is_for(gpu):
    """The default frame of inw01_mixed_moving on a device scene: no sphere records (the 7-float4
    records), the wide walk over 2 time-bin trees, a beam list per bin, and blocks rendered by k_inw_sky."""
    sc, o, od, ost = _case("inw01_mixed_moving")
    d = _Dev(sc)
    try:
        g, gd, ctr, path, sky = d.frame(sc)
    finally:
        d.free()
    print(path, sky)
    assert compare(g, o)["exact_frac"] == 1.0 and compare(gd, od)["exact_frac"] == 1.0
    assert _ray_counters(ctr) == [ost[k] for k in RAY_COUNTERS]
    assert path["kernel"].startswith("k_inw_pm") and path["wide_walk"] == 1
    assert path["sphere_records"] == 0
    assert path["time_bins"] == 2
    assert path["beams"] == 1 and path["beam_bins"] > 1
    assert sky[0] > 0 and sky[1] > 0 and sky[2] == 12 * 8


@pytest.mark.parametrize("name,wide", [(n, 1) for n in MIXED_CASES] + [(n, 0) for n in SHRUNK_CASES] +
                         [("inw01_random", 1), ("inw01_touching_cuboids", 1), ("inw01_dense_glass", 1),
                          ("inw04_cornell", 1), ("inw04_refset", 1)])
def test_wide_walk_follows_the_boxes(gpu, name, wide):
    """Scenes whose objects lie inside their leaf boxes (every scene the packers produce) keep the wide
    walk; the shrunk caller boxes, which the objects stick out of, turn it off for the scene."""
    sc = CASES[name]()
    d = _Dev(sc)
    try:
        path = d.frame(sc)[3]
    finally:
        d.free()
    assert path["wide_walk"] == wide, path


@pytest.mark.parametrize("name,make", [("inw01_mixed_moving", _mixed01), ("inw04_mixed_moving", _mixed04)])
def test_motion_matters(gpu, name, make):
    """The same objects with every last_position = position: the GPU frame differs from the moving one
    in at least 5% of the hit pixels (and equals the oracle's static frame)."""
    sc = _case(name)[0]
    g, _ = _default(name)
    still = make(static=True)
    h, _ = _render(still, {})
    o, od, _ = O.render(still)
    assert compare(h[..., 0:4], o)["exact_frac"] == 1.0 and compare(h[..., 4], od)["exact_frac"] == 1.0
    hit = g[..., 4] < g[..., 4].max()
    differs = ((g[..., 0:4].view(np.uint32) != h[..., 0:4].view(np.uint32)) &
               ~(np.isnan(g[..., 0:4]) & np.isnan(h[..., 0:4]))).any(axis=2)
    frac = (differs & hit).sum() / hit.sum()
    print(name, "hit pixels that differ without motion", frac)
    assert frac >= 0.05


def _chain(scenes, sphere_records, oracles, device_build):
    """One device scene created from scenes[0] and updated to each further one in turn: after every step
    its frame and ray-level counters equal a fresh scene's of the same geometry and the oracle's, and
    rt_debug_path's sphere_records follows the geometry."""
    d = _Dev(scenes[0])
    try:
        for step, (sc, sph, (o, od, ost)) in enumerate(zip(scenes, sphere_records, oracles)):
            if step:
                d.update(sc, device_build)
            g, gd, ctr, path, _ = d.frame(sc)
            f = _Dev(sc)
            try:
                h, hd, hctr, hpath, _ = f.frame(sc)
            finally:
                f.free()
            assert compare(g, h)["exact_frac"] == 1.0 and compare(gd, hd)["exact_frac"] == 1.0, step
            assert _ray_counters(ctr) == _ray_counters(hctr), step
            assert path["sphere_records"] == hpath["sphere_records"] == sph, (step, path)
            assert path["wide_walk"] == hpath["wide_walk"] == 1, (step, path)
            assert compare(g, o)["exact_frac"] == 1.0 and compare(gd, od)["exact_frac"] == 1.0, step
            assert _ray_counters(ctr) == [ost[k] for k in RAY_COUNTERS], step
    finally:
        d.free()


_chains = {}


def _chain_scenes(layout):
    if layout not in _chains:
        if layout == 1:
            mixed = CASES["inw01_mixed_moving"]()
            a = R.make_scene(R.PRESET_INW01_RANDOM, 1234, 600, width=64, height=36, spp=mixed.params.spp)
            oa, om = O.render(a), O.render(mixed)
            _chains[layout] = ([a, mixed, a, mixed], [1, 0, 1, 0], [oa, om, oa, om])
        else:
            mixed = CASES["inw04_mixed_moving"]()
            a = R.make_scene(R.PRESET_INW04_REFSET, width=48, height=48, spp=mixed.params.spp)
            oa, om = O.render(a), O.render(mixed)
            _chains[layout] = ([a, mixed, a], [0, 0, 0], [oa, om, oa])
    return _chains[layout]


@pytest.mark.parametrize("device_build", [False, True])
def test_updates_between_sphere_and_general_records(gpu, device_build):
    """600 moving spheres (sphere records on) -> the mixed scene -> the spheres -> the mixed scene, with
    the caller's nodes and with nodes = NULL and the device build: the sphere records go away and come
    back (1, 0, 1, 0)."""
    _chain(*_chain_scenes(1), device_build)


@pytest.mark.parametrize("device_build", [False, True])
def test_updates_between_inw04_scenes(gpu, device_build):
    """The INW-04 reference set (static, 2 lights) -> inw04_mixed_moving (moving lights) -> back."""
    _chain(*_chain_scenes(4), device_build)
