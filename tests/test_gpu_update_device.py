"""rt_dev_scene_inw_update_device and rt_inw_swept_boxes_async: an INW device scene updated from records,
boxes and lights that live in device memory (torch tensors), with the time-bin trees built on the device.
After it the scene has every structure a fresh one has: the structures are checked directly
(tests/walk_struct_ref.py over rt_debug_walk_dump), the records byte for byte against the host's, frames
and queries bit for bit against a fresh host-built scene of the same records.  Scenes: tests/
walk_struct_cases.py (2 to 2000 objects) and the frames of tests/cases.py."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import cases as frames
import rt_amd as R
import walk_struct_cases as K
import walk_struct_ref as W

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

BINS, NO_BINS = R.RT_UPDATE_BINS, R.RT_UPDATE_NO_BINS
FW, FH, FSPP = 48, 32, 4
_cache = {}


# ---------------------------------------------------------------------------------------- helpers
def _n_lights(c):
    return 0 if c.lights is None else len(c.lights)


def _scene(c, textures=None, **opts):
    """A device scene built from the case on the host (rt_dev_scene_inw_tex), FSPP samples."""
    arr, keep = R.texture_array(textures or [])
    with R.options(**opts):
        s = R.load().rt_dev_scene_inw_tex(R.fptr(c.geom), c.n, c.layout, R.fptr(c.nodes), R.fptr(c.lights), _n_lights(c),
                                          arr if textures else None, len(textures or []), FSPP, -1)
    del keep
    assert s
    return s


def _other(c, name=""):
    """A case of other geometry and the same record layout (the layout is fixed at creation)."""
    return K.case("refset5" if c.layout == 4 else "random5" if name == "grid9" else "grid9")


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32).copy()).cuda()


def _update_dev(s, c, flags=BINS, expect=R.RT_OK, aabbs=None):
    """rt_dev_scene_inw_update_device from torch tensors on the current stream."""
    g, a, l = _dev(c.geom), _dev(c.aabbs if aabbs is None else aabbs), _dev(c.lights)
    tm = (C.c_double * 4)()
    rc = R.load().rt_dev_scene_inw_update_device(s, g.data_ptr(), c.n, a.data_ptr(), None if l is None else l.data_ptr(),
                                                 _n_lights(c), flags, torch.cuda.current_stream().cuda_stream, tm)
    assert rc == expect, rc
    return list(tm)


def _update_host(s, c):
    rc = R.load().rt_dev_scene_inw_update(s, R.fptr(c.geom), c.n, None, R.fptr(c.aabbs), R.fptr(c.lights), _n_lights(c),
                                          None)
    assert rc == 0, rc


def _check_dump(d, c, build):
    """Every INW check on a dump of case c; the leaf-box and rank checks take the dumped LBVH."""
    n = c.n
    assert d["n"] == n and d["build"] == build, d["wide_info"]
    assert d["lbvh"].shape == (2 * n - 1, 8) and d["leafbox"].shape == (n, 8) and d["rank"].shape == (2, n)
    assert len(d["wnodes"]) == len(d["cnodes"]) == len(d["qnodes"]) >= d["n_wtree0"] >= 1
    assert d["wide_info"][0] == d["n_wtree0"] and d["wide_info"][2] == d["depth"]
    leaf = W.lbvh_leaves(d["lbvh"], n)
    assert (leaf >= 0).all() and d["lbvh"][leaf, 0:6].tobytes() == c.aabbs.tobytes()
    assert d["ri_grid"] == c.ri_grid, "the RI grid is built / dropped against the expectation"
    res = W.inw_checks(d, d["lbvh"], n, K.qmargin())
    assert ("ri_grid" in res) == bool(c.ri_grid) and "compact" in res and "quantised" in res
    assert W.reported(res) == {}, {k: v[:3] for k, v in res.items() if v}


def _check_ri_equals_host(d, n):
    """The device RI grid against ri_grid_build over the same (dumped) leaf boxes: equal frame, equal
    offsets, equal id sets per cell (the device fill is atomic: no order within a cell)."""
    h = R.inw_host_dump(d["lbvh"], n)
    assert h is not None and h["ri_grid"] == d["ri_grid"]
    assert h["leafbox"].tobytes() == d["leafbox"].tobytes()
    if not d["ri_grid"]:
        return
    assert list(h["ri_dim"]) == list(d["ri_dim"])
    for k in ("ri_lo", "ri_hi", "ri_inv"):
        assert h[k].tobytes() == d[k].tobytes(), k
    assert np.array_equal(h["ri_cells"], d["ri_cells"])
    cells = d["ri_cells"].astype(np.int64)
    key = np.repeat(np.arange(len(cells) - 1), np.diff(cells))
    for ids in (h["ri_ids"], d["ri_ids"]):
        assert len(ids) == cells[-1]
    assert np.array_equal(h["ri_ids"][np.lexsort((h["ri_ids"], key))], d["ri_ids"][np.lexsort((d["ri_ids"], key))])


def _check_bins(d, c, bins):
    """The layout of `bins` time-bin trees after the swept tree, each tree against the library's own bin
    boxes and against the objects themselves, and the padding."""
    assert d["wbins"] == bins and d["wbin_stride"] >= 1
    n0, stride = d["n_wtree0"], d["wbin_stride"]
    assert len(d["wnodes"]) == n0 + bins * stride
    links = W.links_of(d["wnodes"])
    reach = np.zeros(len(d["wnodes"]), bool)
    for b in range(bins):
        root = 1 + n0 + b * stride
        v = W.check_wide_tree(d["wnodes"], root, c.n, K.bin_boxes(c.geom, c.n, bins, b), wbound=d["wbound"])
        assert v == [], (b, v[:3])
        own = W.inw_sample_boxes(c.geom, (b / bins, (b + 1) / bins), W.unit_dirs(100))
        v = W.check_wide_tree(d["wnodes"], root, c.n, own)
        assert v == [], (b, v[:3])
        # the tree's nodes: breadth first from its root, so the contiguous run its links span
        first = root - 1
        lk = links[first:first + stride]
        inner = lk[(lk > 0) & (lk != 1000000000)]
        assert ((inner > first) & (inner <= first + stride)).all(), b  # links stay inside the tree's stride
        last = int(inner.max()) - 1 if len(inner) else first
        reach[first:last + 1] = True
    pad = d["wnodes"][n0:][~reach[n0:]]
    assert (pad[:, 0:36] == np.float32(1e30)).all() and (pad[:, 36:40].view(np.int32) == 1000000000).all()
    # the largest tree fills its stride
    assert max(int(np.flatnonzero(reach[n0 + b * stride:n0 + (b + 1) * stride]).max()) + 1 for b in range(bins)) == stride


def _updated_dump(name, flags=BINS, **opts):
    c = K.case(name)
    s = _scene(_other(c, name), **opts)
    try:
        _update_dev(s, c, flags)
        return c, R.walk_dump_all(s)
    finally:
        R.load().rt_dev_scene_free(s)


# ------------------------------------------------------------------------------ 1-3: structures
@pytest.mark.parametrize("name", K.NAMES)
def test_device_update_builds_every_structure(gpu, name):
    """A scene of other geometry updated to the case from device tensors with RT_UPDATE_BINS: every INW
    check on the dump, the RI grid equal to the host's, and for a moving scene two time-bin trees."""
    c, d = _updated_dump(name)
    _check_dump(d, c, c.build)
    _check_ri_equals_host(d, c.n)
    assert d["wbins"] == (2 if c.moving else 1)
    if c.moving:
        _check_bins(d, c, 2)
    else:
        assert d["wbin_stride"] == 0 and len(d["wnodes"]) == d["n_wtree0"]


@pytest.mark.parametrize("bins", [4, 16])
@pytest.mark.parametrize("name", ["random600", "mixed250"])
def test_more_time_bins(gpu, name, bins):
    c, d = _updated_dump(name, inw_time_bins=bins)
    _check_dump(d, c, c.build)
    _check_bins(d, c, bins)


@pytest.mark.parametrize("name", ["random600", "mixed120_l4", "random3"])
def test_no_bins_equals_the_host_pointer_update(gpu, name):
    """RT_UPDATE_NO_BINS: the swept tree alone, and the structures that do not depend on atomics' order
    byte-equal to rt_dev_scene_inw_update's for the same case."""
    c, d = _updated_dump(name, NO_BINS)
    assert d["wbins"] == 1 and d["wbin_stride"] == 0 and len(d["wnodes"]) == d["n_wtree0"]
    _check_dump(d, c, c.build)
    s = _scene(_other(c, name))
    try:
        _update_host(s, c)
        h = R.walk_dump_all(s)
    finally:
        R.load().rt_dev_scene_free(s)
    _check_dump(h, c, c.build)
    for k in ("lbvh", "leafbox", "rank"):
        assert d[k].tobytes() == h[k].tobytes(), k
    assert d["dfs_high"] == h["dfs_high"]


# ------------------------------------------------------------------------------------ 4: records
@pytest.mark.parametrize("name", ["random600", "mixed250", "mixed120_l4", "cornell"])
def test_records_equal_the_hosts(gpu, name):
    """The hot, cold and sphere records k_inw_prepare writes against a fresh host-built scene's."""
    c, d = _updated_dump(name)
    s = _scene(c)
    try:
        f = R.walk_dump_all(s)
    finally:
        R.load().rt_dev_scene_free(s)
    assert f["hot"].shape == (c.n, 28) and f["cold"].shape == (c.n, 8)
    assert d["hot"].tobytes() == f["hot"].tobytes()
    assert d["cold"].tobytes() == f["cold"].tobytes()
    sph = np.zeros((c.n, 12), np.float32)
    is_sph = R.load().rt_debug_sphere_records(R.fptr(c.geom), c.n, c.layout, R.fptr(sph))
    assert (d["sph"] is not None) == bool(is_sph) == (f["sph"] is not None)
    if is_sph:
        assert d["sph"].tobytes() == f["sph"].tobytes() == sph.tobytes()


# ------------------------------------------------------------------------- 5: frames and queries
def _small(sc):
    p = R.RtParams.from_buffer_copy(bytes(sc.params))
    p.width, p.height, p.spp = FW, FH, FSPP
    return dataclasses.replace(sc, params=p)


def _frame_scene(name):
    """A packed scene with camera and parameters (FW x FH, FSPP samples) and its textures."""
    if name not in _cache:
        if name == "random600":
            sc = R.make_scene(R.PRESET_INW01_RANDOM, 1234, 600, width=FW, height=FH, spp=FSPP)
        elif name == "mixed120_l4":
            sc = _small(frames.CASES["inw04_mixed_moving"]())
        else:  # the INW-04 reference set with three textures on five of its objects
            sc = _small(frames.CASES["inw04_refset"]())
            for i, t in enumerate([1, 2, 3, 0, 2]):
                sc.geom[i % sc.n, 27] = float(t)
            rng = np.random.default_rng(11)
            sc.textures = [rng.integers(0, 256, (40, 64, 3)).astype(np.uint8),
                           rng.integers(0, 256, (17, 33, 4)).astype(np.uint8),
                           rng.integers(0, 256, (8, 8, 3)).astype(np.uint8)]
        _cache[name] = sc
    return _cache[name]


def _case_of(sc):
    return K.Case("frame", np.ascontiguousarray(sc.geom, np.float32), np.ascontiguousarray(sc.aabbs, np.float32),
                  layout=sc.layout, lights=sc.lights if sc.n_lights else None,
                  _nodes=np.ascontiguousarray(sc.nodes, np.float32))


def _frame(s, sc, expect=R.RT_OK):
    """One frame of device scene s with sc's camera and params: colour, depth, the six counters."""
    p = sc.params
    img = torch.zeros((p.height, p.width, 4), dtype=torch.float32, device="cuda")
    dep = torch.zeros((p.height, p.width), dtype=torch.float32, device="cuda")
    ctr = torch.zeros(6, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    rc = R.load().rt_render_image_async(s, C.byref(sc.camera), C.byref(p), img.data_ptr(), dep.data_ptr(), ctr.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream)
    assert rc == expect, rc
    torch.cuda.synchronize()
    return img.cpu().numpy().tobytes(), dep.cpu().numpy().tobytes(), [int(x) for x in ctr.cpu().numpy()]


def _rays(c, n=300, seed=3):
    """n rays from a sphere around the scene towards its objects, at random time ratios."""
    rng = np.random.default_rng(seed)
    mid = c.geom[:, 0:3].astype(np.float64).mean(axis=0)
    rad = 1.5 * float(np.abs(c.geom[:, 0:3] - mid).max()) + 5.0
    u = rng.normal(size=(n, 3))
    o = mid + rad * u / np.linalg.norm(u, axis=1, keepdims=True)
    to = c.geom[rng.integers(0, c.n, n), 0:3] + rng.normal(scale=0.3, size=(n, 3))
    dd = to - o
    dd /= np.linalg.norm(dd, axis=1, keepdims=True)
    rays = np.zeros(n, R.RAY_DTYPE)
    rays["o"], rays["d"], rays["tmax"], rays["ratio"] = o, dd, 1e30, rng.uniform(0, 1, n)
    pr = np.zeros(n, R.PATH_RAY_DTYPE)
    pr["o"], pr["d"], pr["sample"] = o, dd, rng.integers(0, FSPP, n)
    return rays, pr


def _queries(s, c):
    """Closest-hit and path answers (both child orders) of a few hundred rays, as bytes."""
    lib = R.load()
    rays, pr = _rays(c)
    d_rays = torch.from_numpy(np.frombuffer(rays.tobytes(), np.uint8).copy()).cuda()
    d_pr = torch.from_numpy(np.frombuffer(pr.tobytes(), np.uint8).copy()).cuda()
    out = []
    st = torch.cuda.current_stream().cuda_stream
    for flags in (0, R.RT_TRACE_INVERT):
        d_hits = torch.zeros(len(rays) * 32, dtype=torch.uint8, device="cuda")
        d_out = torch.zeros(len(rays) * 32, dtype=torch.uint8, device="cuda")
        assert lib.rt_trace_rays_async(s, d_rays.data_ptr(), len(rays), flags, d_hits.data_ptr(), None, st) == R.RT_OK
        assert lib.rt_path_rays_async(s, d_pr.data_ptr(), len(pr), 6, flags, d_out.data_ptr(), None, st) == R.RT_OK
        torch.cuda.synchronize()
        out.append((d_hits.cpu().numpy().tobytes(), d_out.cpu().numpy().tobytes()))
    hits = np.frombuffer(out[0][0], R.HIT_DTYPE)
    assert (hits["id"] >= 0).sum() > len(rays) // 4  # the rays do hit the scene
    return out


def _assert_as_fresh(s, sc, c, what, **opts):
    """Frame and queries of the updated handle s against a fresh host-built scene of the same records."""
    f = _scene(c, textures=getattr(sc, "textures", None), **opts)
    try:
        want, want_q = _frame(f, sc), _queries(f, c)
    finally:
        R.load().rt_dev_scene_free(f)
    got = _frame(s, sc)
    assert got[0] == want[0], what + ": colour"
    assert got[1] == want[1], what + ": depth"
    assert [got[2][k] for k in (0, 3, 4, 5)] == [want[2][k] for k in (0, 3, 4, 5)], what
    assert _queries(s, c) == want_q, what + ": queries"


@pytest.mark.parametrize("wide", [1, 0])
@pytest.mark.parametrize("name", ["random600", "mixed120_l4", "refset_tex"])
def test_frames_and_queries_equal_a_fresh_scenes(gpu, name, wide):
    sc = _frame_scene(name)
    c = _case_of(sc)
    tex = getattr(sc, "textures", None)
    s = _scene(_other(c), textures=tex, inw_wide_walk=wide)
    try:
        _update_dev(s, c)
        _assert_as_fresh(s, sc, c, name, inw_wide_walk=wide)
        if wide and c.moving:
            assert R.debug_path(s)["time_bins"] == 2
    finally:
        R.load().rt_dev_scene_free(s)


# --------------------------------------------------------------------- 6: a device-to-device loop
def test_device_to_device_loop(gpu):
    """Three steps: a torch expression moves the objects on the device, rt_inw_swept_boxes_async makes
    their boxes, the update and a frame follow on the same stream without a synchronisation in between.
    Each frame equals the frame of a fresh host-built scene of the read-back records over R.lbvh_build of
    the read-back boxes; the boxes hold the objects over the shutter interval."""
    sc = _frame_scene("random600")
    n = sc.n
    s = _scene(_case_of(sc))
    geom = _dev(sc.geom)
    boxes = torch.zeros((n, 6), dtype=torch.float32, device="cuda")
    step = torch.from_numpy(np.random.default_rng(5).uniform(-0.3, 0.3, (n, 3)).astype(np.float32)).cuda()
    try:
        for k in range(3):
            delta = step * float(k + 1) * 0.5
            geom[:, 0:3] += delta
            geom[:, 15:18] = delta
            R.inw_swept_boxes(geom, n, boxes, torch.cuda.current_stream().cuda_stream)
            R.update_inw_device(s, geom, n, boxes, flags=BINS, stream=torch.cuda.current_stream().cuda_stream)
            g, b = geom.cpu().numpy(), boxes.cpu().numpy()
            own = W.inw_sample_boxes(g, (0.0, 1.0), W.unit_dirs(100))
            assert (b[:, 0:3] <= own[:, 0:3]).all() and (b[:, 3:6] >= own[:, 3:6]).all(), k
            assert R.inw_stick_out(g, aabbs=b) <= 1.0
            assert b.tobytes() == K.bin_boxes(g, n, 1, 0).tobytes()  # the bin-box formula with one bin
            c = K.Case("step", g, b)
            _assert_as_fresh(s, sc, c, f"step {k}")
            assert R.debug_path(s)["time_bins"] == 2
    finally:
        R.load().rt_dev_scene_free(s)


# ---------------------------------------------------------------------------------- 7: decisions
def test_decisions_follow_the_hosts_rules(gpu):
    sc = _frame_scene("random600")
    c = _case_of(sc)
    lib = R.load()
    s = _scene(K.case("grid9"))
    try:
        # one object sticks out of its caller box by 10 margins: no wide walk, the same frame
        a = c.aabbs.copy()
        f = c.geom[7].astype(np.float64)
        assert int(f[18] + 0.1) == 1  # an ellipsoid: its +x extent is sqrt(sum_c (M_c0 s_c)^2)
        ext = np.sqrt(sum((f[3 + 3 * k] * f[12 + k]) ** 2 for k in range(3)))
        reach = max(f[0], f[0] - f[15]) + ext
        a[7, 3] = np.float32(reach - 10.0 * 1e-5 * max(1.0, float(np.abs(a[7]).max())))
        out = K.Case("out", c.geom, a)
        assert 5.0 < R.inw_stick_out(out.geom, aabbs=out.aabbs) < 20.0
        _update_dev(s, out)
        d = R.walk_dump_all(s)
        assert d["wide_info"][0] == 0 and d["wbins"] == 1 and len(d["wnodes"]) == 0
        _assert_as_fresh(s, sc, out, "stick-out")
        # a NaN position does the same
        g = c.geom.copy()
        g[11, 1] = np.nan
        nan = K.Case("nan", g, c.aabbs)
        _update_dev(s, nan)
        assert R.walk_dump_all(s)["wide_info"][0] == 0
        fr = _scene(nan)
        try:
            want = _frame(fr, sc)
        finally:
            lib.rt_dev_scene_free(fr)
        got = _frame(s, sc)
        assert got[0:2] == want[0:2] and [got[2][k] for k in (0, 3, 4, 5)] == [want[2][k] for k in (0, 3, 4, 5)]
        # back to the plain case: the wide walk returns
        _update_dev(s, c)
        assert R.walk_dump_all(s)["wbins"] == 2
    finally:
        lib.rt_dev_scene_free(s)
    # inw_time_bins = 0: no bin trees whatever the flags
    s = _scene(K.case("grid9"), inw_time_bins=0)
    try:
        _update_dev(s, c)
        d = R.walk_dump_all(s)
        assert d["wbins"] == 1 and len(d["wnodes"]) == d["n_wtree0"] >= 1
    finally:
        lib.rt_dev_scene_free(s)
    # a TextureIndex of 3 on a scene with no texture bound: the render refuses
    l4 = _frame_scene("mixed120_l4")
    c4 = _case_of(l4)
    g = c4.geom.copy()
    g[5, 27] = 3.0
    s = _scene(K.case("refset5"))
    try:
        _update_dev(s, K.Case("tex", g, c4.aabbs, layout=4, lights=c4.lights))
        _frame(s, l4, expect=R.RT_E_UNSUPPORTED)
        _update_dev(s, c4)
        _assert_as_fresh(s, l4, c4, "after the textured records")
    finally:
        lib.rt_dev_scene_free(s)


# ------------------------------------------------------------------------------------ 8: fallback
def test_past_the_level_cap_the_host_builds(gpu):
    c = K.case("random600")
    lib = R.load()
    s = _scene(K.case("grid9"))
    try:
        assert lib.rt_debug_build_level_cap(4) == 0
        _update_dev(s, c)
        d = R.walk_dump_all(s)
    finally:
        lib.rt_debug_build_level_cap(0)
        lib.rt_dev_scene_free(s)
    _check_dump(d, c, 2)
    _check_bins(d, c, 2)


# ---------------------------------------------------------------------------------- 9: no remnant
def test_updates_leave_no_remnant(gpu):
    """One scene through six updates, the two entry points in turn: fewer objects, more than its buffers
    held, the pile that drops the RI grid, five objects, a static scene.  Every dump refers to the new
    scene alone."""
    lib = R.load()
    s = _scene(K.case("grid9"))
    try:
        for i, name in enumerate(("random600", "random257", "random1025", "dups300", "random5", "coplanar400")):
            c = K.case(name)
            if i % 2 == 0:
                _update_dev(s, c)
            else:
                _update_host(s, c)
            d = R.walk_dump_all(s)
            _check_dump(d, c, c.build)
            if i % 2 == 0 and c.moving:
                _check_bins(d, c, 2)
            else:
                assert d["wbins"] == 1 and d["wbin_stride"] == 0 and len(d["wnodes"]) == d["n_wtree0"], name
            assert d["hot"].shape == (c.n, 28) and d["hot"][:, 0:18].tobytes() == c.geom[:, 0:18].tobytes()
            if c.ri_grid:
                assert d["ri_cells"][-1] == len(d["ri_ids"]) and d["ri_ids"].max() < c.n
            else:
                assert d["ri_cells"] is None and d["wide_info"][4] == 0
    finally:
        lib.rt_dev_scene_free(s)


# -------------------------------------------------------------------------------------- 10: errors
def test_errors_leave_the_scene_as_it_was(gpu):
    lib = R.load()
    sc = _frame_scene("random600")
    c = _case_of(sc)
    s = _scene(c)
    try:
        before = _frame(s, sc)
        for flags in (12, 16):
            _update_dev(s, K.case("random257"), flags, expect=R.RT_E_ARG)
            assert _frame(s, sc) == before, flags
    finally:
        lib.rt_dev_scene_free(s)
    iow = R.make_scene(R.PRESET_IOW03_FINAL, 20250131, 0, width=FW, height=FH, spp=FSPP)
    s = R.dev_scene(iow, FSPP)
    try:
        _update_dev(s, c, expect=R.RT_E_UNSUPPORTED)
        p = iow.params
        img = torch.zeros((p.height, p.width, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        assert lib.rt_render_image_async(s, C.byref(iow.camera), C.byref(p), img.data_ptr(), None, None,
                                         torch.cuda.current_stream().cuda_stream) == R.RT_OK
        torch.cuda.synchronize()
        assert float(img.abs().sum()) > 0
    finally:
        lib.rt_dev_scene_free(s)


def test_new_kernels_spill_nothing(gpu):
    for which, name in enumerate(R.UPDATE_KERNELS):
        info = R.update_kernel_info(which)
        print(name, info)
        assert info["scratch_bytes"] == 0 and info["vgprs"] > 0, (name, info)
