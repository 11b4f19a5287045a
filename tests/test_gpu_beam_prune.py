"""Beam-list pruning (rt_options.inw_beam_prune, DESIGN.md §5.2 "Pixel beams"): k_inw_beam leaves out
of a pixel's list the leaves no primary ray of the pixel can touch -- by the beam's radius over the
leaf's own depth interval (1) and, with sphere records, by the sphere's swept centre (2).  A dropped
object was never hit, so every frame must come out bit for bit as with the unpruned lists (0) and as
the CPU oracle renders it: colour, depth, and the ray-level counters.  rt_debug_beam_lists reads the
lists back, so the cases also show that lists were in fact shortened (or, for the dense case, cut).

Every render here goes through a device scene (the hook needs one); the oracle renders each scene
once."""
import ctypes as C
import functools

import numpy as np
import pytest

import rt_amd as R
from cases import _scene_cam, compare
from oracle import oracle as O

pytestmark = pytest.mark.gpu

RAY_COUNTERS = ("segments", "stack_drops", "nan_drops")
COUNTER_AT = {"segments": 0, "node_visits": 1, "prim_tests": 2, "shadow_queries": 3, "stack_drops": 4, "nan_drops": 5}
INW1 = (R.PRESET_INW01_RANDOM, 1234, 3000)
INW4 = (R.PRESET_INW04_CORNELL, 7, 0)
SCENES = {
    "inw1": lambda: R.make_scene(*INW1, width=192, height=108, spp=24),
    "inw1_ragged": lambda: R.make_scene(*INW1, width=97, height=43, spp=7),
    "inw4": lambda: R.make_scene(*INW4, width=128, height=128, spp=16),
    # a lens of radius 0.5 focused 9 units past its tip: the beam is wide everywhere but at the focus
    "inw1_wide_near": lambda: _scene_cam(*INW1, {"aperture": 1.0, "focus_dist": 10.0}, width=80, height=45, spp=12),
    # a lens of radius 2: the unpruned lists overflow their 32 entries
    "inw1_dense": lambda: _scene_cam(*INW1, {"aperture": 4.0}, width=64, height=36, spp=12),
    "inw1_tiles": lambda: R.make_scene(*INW1, width=100, height=60, spp=12),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    sc = SCENES[name]()
    return sc, O.render(sc)


def _same(a, b):
    return compare(a, b)["exact_frac"] == 1.0


def _make(sc, opts):
    lib = R.load()
    with R.options(**opts):
        lights = sc.lights if sc.n_lights else None
        s = lib.rt_dev_scene_inw(R.fptr(sc.geom), sc.n, sc.layout, R.fptr(sc.nodes), R.fptr(lights), sc.n_lights,
                                 sc.params.spp, -1)
    assert s
    return s


def _lists(s, entries=False):
    """rt_debug_beam_lists: (totals dict, counts, cuts, entries or None)."""
    lib = R.load()
    tot = (C.c_uint64 * 8)()
    assert lib.rt_debug_beam_lists(s, tot, None, None, None, 0) == 0
    lists, cap = int(tot[0]), int(tot[5])
    n, cut = np.zeros(max(lists, 1), np.uint32), np.zeros(max(lists, 1), np.float32)
    ent = np.zeros((max(lists, 1), max(cap, 1)), np.uint64) if entries else None
    assert lib.rt_debug_beam_lists(s, tot, n.ctypes.data_as(C.POINTER(C.c_uint32)), R.fptr(cut),
                                   ent.ctypes.data_as(C.POINTER(C.c_uint64)) if entries else None, lists) == 0
    t = dict(zip(("lists", "nonempty", "entries", "cut", "off", "cap"), (int(v) for v in tot[:6])))
    return t, n[:lists], cut[:lists], ent[:lists] if entries else None


def _render(sc, opts, entries=False):
    """One frame of a fresh device scene built and rendered under `opts`."""
    import torch

    lib = R.load()
    p = sc.params
    s = _make(sc, opts)
    try:
        img = torch.zeros((p.height, p.width, 4), dtype=torch.float32, device="cuda")
        dep = torch.zeros((p.height, p.width), dtype=torch.float32, device="cuda")
        ctr = torch.zeros(6, dtype=torch.int64, device="cuda")
        assert lib.rt_render_image_async(s, C.byref(sc.camera), C.byref(p), img.data_ptr(), dep.data_ptr(),
                                         ctr.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        c = ctr.cpu().numpy()
        return {"rgba": img.cpu().numpy(), "depth": dep.cpu().numpy(),
                "st": {k: int(c[i]) for k, i in COUNTER_AT.items()}, "path": R.debug_path(s),
                "sky": R.debug_sky_blocks(s), "lists": _lists(s, entries)}
    finally:
        lib.rt_dev_scene_free(s)


def _parity(name, opts, shrinks=True):
    """The three prune levels of one case under `opts`: each equal to the oracle and to level 0.
    shrinks: the scene has many small objects, so level 1 must shorten the lists (not vacuous)."""
    sc, (o, od, ost) = _case(name)
    arms = {p: _render(sc, {**opts, "inw_beam_prune": p}) for p in (0, 1, 2)}
    for p, a in arms.items():
        path, tot = a["path"], a["lists"][0]
        print(name, opts, "prune", p, "->", path["beam_prune"], tot, "sky", a["sky"],
              {k: a["st"][k] for k in ("segments", "prim_tests")})
        assert _same(a["rgba"], o) and _same(a["depth"], od), (name, opts, p)
        assert _same(a["rgba"], arms[0]["rgba"]) and _same(a["depth"], arms[0]["depth"])
        for k in RAY_COUNTERS:
            assert a["st"][k] == ost[k] == arms[0]["st"][k], (k, p, a["st"][k], ost[k])
        # what the frame reports: the level asked for, step 2 only with sphere records, 0 without lists
        want = 0 if not path["beams"] else (min(p, 1) if not path["sphere_records"] else p)
        assert path["beam_prune"] == want, (p, path)
        assert (tot["lists"] > 0) == bool(path["beams"])
    assert arms[0]["path"]["beams"] == 1 and arms[0]["lists"][0]["entries"] > 0
    e = [arms[p]["lists"][0]["entries"] for p in (0, 1, 2)]
    assert e[2] <= e[1] <= e[0] and (e[1] < e[0] or not shrinks), e
    assert arms[2]["sky"][0] >= arms[1]["sky"][0] >= arms[0]["sky"][0]
    return arms


@pytest.mark.parametrize("name,opts", [
    ("inw1", {}),
    ("inw1_ragged", {}),
    ("inw4", {"inw_order": 1}),        # forced pixel-major; cuboids, no sphere records: step 1 only
    ("inw1_wide_near", {}),
])
def test_parity(gpu, name, opts):
    arms = _parity(name, opts, shrinks=name.startswith("inw1"))  # (the Cornell box: a few large cuboids)
    if name.startswith("inw1"):  # sphere records: step 2 drops more
        assert arms[2]["lists"][0]["entries"] < arms[1]["lists"][0]["entries"]


@pytest.mark.parametrize("opts", [
    {"inw_beam_bins": 0},                      # one list per pixel over the swept boxes (K = 1)
    {"inw_time_bins": 0},                      # no bin trees at all
    {"inw_time_bins": 5},                      # five lists per pixel, uneven sample splits (7 spp)
    {"inw_sphere_records": 0},                 # the box path only
    {"inw_beams": 2},                          # (id, t) pairs
    {"inw_sky_blocks": 0},
    {"inw_sky_blocks": 1},
    {"inw_sky_blocks": 0, "inw_time_bins": 5, "inw_beams": 2},
], ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_parity_matrix(gpu, opts):
    arms = _parity("inw1_ragged", opts)
    bins = opts.get("inw_time_bins", 2)
    assert arms[2]["path"]["beam_bins"] == (bins if bins > 1 and opts.get("inw_beam_bins", 1) else 0)
    if opts.get("inw_sphere_records", 1) == 0:
        assert arms[2]["lists"][0] == arms[1]["lists"][0]  # level 2 has nothing more to go on


def test_parity_dense_lists_cut(gpu):
    """With the unpruned lists some overflow the 32 entries (asserted), so their cut decides where a
    ray must fall back to the walk; the pruned lists are cut at a later key or not at all."""
    arms = _parity("inw1_dense", {})
    t0, n0, cut0, _ = arms[0]["lists"]
    assert t0["cut"] > 0 and int((n0 == t0["cap"]).sum()) > 0, t0
    for p in (1, 2):
        tp, _, cutp, _ = arms[p]["lists"]
        assert (cutp >= cut0).all()
        assert tp["cut"] <= t0["cut"]


def test_parity_tiles(gpu):
    """rt_render_tiles_async, every other 16 x 16 tile of a 100 x 60 frame (ragged tiles at the right
    and bottom edges), one device scene, the prune level switched by rt_dev_scene_set_options."""
    import torch

    sc, (o, od, _) = _case("inw1_tiles")
    lib = R.load()
    ts = 16
    tiles = [(tx, ty) for ty in range((60 + ts - 1) // ts) for tx in range((100 + ts - 1) // ts)][::2]
    dev = torch.device("cuda")
    d_tiles = torch.tensor(tiles, dtype=torch.int32, device=dev).contiguous()
    s = _make(sc, {})
    seg, ent = {}, {}
    try:
        for p in (0, 1, 2):
            opt = R.default_options()
            opt.inw_beam_prune = p
            assert lib.rt_dev_scene_set_options(s, C.byref(opt)) == 0
            out = torch.zeros((len(tiles), ts, ts, 4), dtype=torch.float32, device=dev)
            dep = torch.zeros((len(tiles), ts, ts), dtype=torch.float32, device=dev)
            ctr = torch.zeros(6, dtype=torch.int64, device=dev)
            assert lib.rt_render_tiles_async(s, C.byref(sc.camera), C.byref(sc.params), d_tiles.data_ptr(), len(tiles),
                                             ts, out.data_ptr(), dep.data_ptr(), ctr.data_ptr(),
                                             torch.cuda.current_stream().cuda_stream) == 0
            torch.cuda.synchronize()
            assert R.debug_path(s)["beam_prune"] == p
            ent[p] = _lists(s)[0]["entries"]
            seg[p] = tuple(int(ctr[COUNTER_AT[k]].item()) for k in RAY_COUNTERS)
            a, d = out.cpu().numpy(), dep.cpu().numpy()
            for i, (tx, ty) in enumerate(tiles):
                hh, ww = min(ts, 60 - ty * ts), min(ts, 100 - tx * ts)
                assert _same(a[i, :hh, :ww], o[ty * ts:ty * ts + hh, tx * ts:tx * ts + ww]), (p, tx, ty)
                assert _same(d[i, :hh, :ww], od[ty * ts:ty * ts + hh, tx * ts:tx * ts + ww]), (p, tx, ty)
    finally:
        lib.rt_dev_scene_free(s)
    print("tiles: entries", ent, "ray counters", seg)
    assert seg[0] == seg[1] == seg[2]
    assert ent[2] < ent[1] < ent[0]


def _is_subsequence(b, a):
    it = iter(a)
    return all(x in it for x in b)


def test_list_structure_on_the_bench_scene(gpu):
    """The bench frame's scene and camera (10k moving spheres) at 240 x 135, 8 spp: what pruning does
    to the lists themselves, read back with rt_debug_beam_lists."""
    sc = R.make_scene(R.PRESET_INW01_RANDOM, 1234, 10_000, width=240, height=135, spp=8)
    arms = {p: _render(sc, {"inw_beam_prune": p}, entries=True) for p in (0, 1, 2)}
    for p in (1, 2):
        assert _same(arms[p]["rgba"], arms[0]["rgba"]) and _same(arms[p]["depth"], arms[0]["depth"])
        for k in RAY_COUNTERS:
            assert arms[p]["st"][k] == arms[0]["st"][k], k
    t0, n0, cut0, e0 = arms[0]["lists"]
    assert t0["lists"] == 2 * 64 * ((240 + 7) // 8) * ((135 + 7) // 8) and t0["nonempty"] > 0
    off0 = n0 == 0xFFFFFFFF
    for p in (1, 2):
        tp, np_, cutp, ep = arms[p]["lists"]
        assert tp["lists"] == t0["lists"] and ((np_ == 0xFFFFFFFF) == off0).all()
        # a list that was empty and complete stays so
        was_empty = (n0 == 0) & np.isinf(cut0)
        assert (np_[was_empty] == 0).all() and np.isinf(cutp[was_empty]).all()
        assert (cutp >= cut0).all()
        # lists complete in both arms: the pruned one is a subsequence, the entry words unchanged
        both = np.nonzero(~off0 & np.isinf(cut0) & np.isinf(cutp) & (n0 > 0))[0]
        assert both.size > 1000
        assert (np_[both] <= n0[both]).all()
        for l in both:
            assert _is_subsequence(ep[l, :np_[l]].tolist(), e0[l, :n0[l]].tolist()), (p, int(l))
    tot = {p: arms[p]["lists"][0] for p in (0, 1, 2)}
    sky = {p: arms[p]["sky"] for p in (0, 1, 2)}
    print("lists", tot, "sky blocks", sky,
          "entry ratios", {p: round(tot[p]["entries"] / tot[0]["entries"], 4) for p in (1, 2)},
          "prim_tests", {p: arms[p]["st"]["prim_tests"] for p in (0, 1, 2)})
    assert tot[2]["entries"] < tot[1]["entries"] < tot[0]["entries"]
    assert tot[2]["nonempty"] <= tot[1]["nonempty"] <= tot[0]["nonempty"]
    assert sky[2][0] >= sky[1][0] >= sky[0][0] and sky[0][0] > 0
    assert arms[2]["st"]["prim_tests"] < arms[0]["st"]["prim_tests"]
