"""Batched path (radiance) queries (rt_path_rays_async / rt_path_inw) on the GPU, bit for bit against
the fixtures tests/golden/paths_*.npz (the CPU oracle's sample loop restarted from each query's ray,
tests/path_ref.c; tests/test_path_ref.py recomputes them): colour, depth, the per-path counts and the
reference's four counters, for both child orders, every scene option, ragged batch sizes, lanes that
take one path after another, updated scenes, and whole frames folded from path queries."""
import ctypes as C

import numpy as np
import pytest

import path_ref as P
import rt_amd as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = 0xCD
REF_COUNTERS = (0, 3, 4, 5)  # segments, shadow queries, dropped pushes, NaN directions: the reference's
STAT_KEYS = ("segments", "node_visits", "prim_tests", "shadow_queries", "stack_drops", "nan_drops")

_cache = {}


def fx(name):
    if name not in _cache:
        _cache[name] = P.load_fixture(name)
    return _cache[name]


def dev_scene(f, spp=None):
    arr, keep = R.texture_array(f.textures or [])
    lights = f.lights if f.n_lights else None
    s = R.load().rt_dev_scene_inw_tex(R.fptr(f.geom), f.n, f.layout, R.fptr(f.nodes), R.fptr(lights), f.n_lights,
                                      arr if f.textures else None, len(f.textures or []), spp or f.spp, -1)
    assert s
    return s


def paths_async(s, rays, max_bounces, flags, n_rays=None, cap=None, counters=True):
    """rt_path_rays_async on the current torch stream; the output buffer (cap records) starts as
    SENTINEL bytes.  Returns (rc, out (cap,), counters (6,))."""
    rays = np.ascontiguousarray(rays, R.PATH_RAY_DTYPE)
    n_rays = len(rays) if n_rays is None else n_rays
    cap = max(len(rays), 1) if cap is None else cap
    dev = torch.device("cuda")
    d_rays = torch.from_numpy(np.frombuffer(rays.tobytes() + bytes(32), np.uint8).copy()).to(dev)
    d_out = torch.full((cap * 32,), SENTINEL, dtype=torch.uint8, device=dev)
    d_ctr = torch.zeros(6, dtype=torch.int64, device=dev)
    rc = R.load().rt_path_rays_async(s, d_rays.data_ptr(), n_rays, max_bounces, flags, d_out.data_ptr(),
                                     d_ctr.data_ptr() if counters else None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, d_out.cpu().numpy().view(R.PATH_OUT_DTYPE), d_ctr.cpu().numpy()


def assert_same(got, want, what):
    assert got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero((got.view(np.uint32).reshape(-1, 8) != want.view(np.uint32).reshape(-1, 8)).any(1))
        raise AssertionError(f"{what}: {len(bad)} of {len(got)} outputs differ, first {bad[0]}: got {got[bad[0]]} "
                             f"want {want[bad[0]]}")


def assert_ref_counters(ctr, want, what):
    for k in REF_COUNTERS:
        assert int(ctr[k]) == int(want[k]), (what, k, int(ctr[k]), int(want[k]))


def stats_list(st):
    return [st[k] for k in STAT_KEYS]


@pytest.mark.parametrize("invert", [0, 1])
@pytest.mark.parametrize("name", P.SCENES)
def test_parity_blocking_and_async(gpu, name, invert):
    f = fx(name)
    want, wctr = f.out[invert], f.ctr[invert]
    out, st = R.paths(f, f.rays, f.max_bounces, invert * R.RT_TRACE_INVERT)
    assert_same(out, want, f"{name} rt_path_inw")
    assert_ref_counters(stats_list(st), wctr, f"{name} rt_path_inw")
    assert st["node_visits"] > 0 and st["prim_tests"] > 0
    s = dev_scene(f)
    try:
        rc, out, ctr = paths_async(s, f.rays, f.max_bounces, invert * R.RT_TRACE_INVERT)
    finally:
        R.load().rt_dev_scene_free(s)
    assert rc == R.RT_OK
    assert_same(out, want, f"{name} rt_path_rays_async")
    assert_ref_counters(ctr, wctr, f"{name} rt_path_rays_async")
    assert ctr[1] > 0 and ctr[2] > 0


def test_batch_sizes_and_untouched_tail(gpu):
    """Prefixes around the 64-query wave claim; records past n_rays keep the sentinel."""
    f = fx("pile100")
    want = f.out[1]
    s = dev_scene(f)
    try:
        for k in (0, 1, 63, 64, 65, 1000, 2047):
            rc, out, ctr = paths_async(s, f.rays, f.max_bounces, R.RT_TRACE_INVERT, n_rays=k, cap=len(f.rays))
            assert rc == R.RT_OK, k
            assert_same(out[:k], want[:k], f"prefix {k}")
            assert np.all(out[k:].view(np.uint8) == SENTINEL), k
            assert ctr[0] == want["segments"][:k].sum() and ctr[4] == want["drops"][:k].sum(), k
    finally:
        R.load().rt_dev_scene_free(s)


@pytest.mark.parametrize("name", ["pile100", "glass600"])
def test_one_block_refills_its_lanes(gpu, name):
    """A grid of one block answers 2,048 queries: every lane takes eight paths on average, one after
    another (with the full grid every lane has exactly one path and the refill never runs)."""
    f = fx(name)
    lib = R.load()
    s = dev_scene(f)
    assert lib.rt_debug_paths_max_blocks(1) == 0
    try:
        for invert in (0, 1):
            rc, out, ctr = paths_async(s, f.rays, f.max_bounces, invert * R.RT_TRACE_INVERT)
            assert rc == R.RT_OK
            assert_same(out, f.out[invert], f"{name} one block, invert {invert}")
            assert_ref_counters(ctr, f.ctr[invert], f"{name} one block")
    finally:
        assert lib.rt_debug_paths_max_blocks(0) == 1
        lib.rt_dev_scene_free(s)


def test_full_grid_refills_its_lanes(gpu):
    """pile100's queries tiled 192 times: 393,216 queries, more than the chip's resident lanes, paths
    of 1 to 285 segments side by side.  Every copy equals the fixture, and a fixed permutation of the
    batch gives the permuted outputs."""
    f = fx("pile100")
    reps = 192
    rays = np.tile(f.rays, reps)
    want = np.tile(f.out[1], reps)
    s = dev_scene(f)
    try:
        rc, out, ctr = paths_async(s, rays, f.max_bounces, R.RT_TRACE_INVERT)
        assert rc == R.RT_OK
        assert_same(out, want, "tiled batch")
        for k in REF_COUNTERS:
            assert int(ctr[k]) == reps * int(f.ctr[1][k]), k
        perm = np.random.default_rng(5).permutation(len(rays))
        rc, out, ctr = paths_async(s, rays[perm], f.max_bounces, R.RT_TRACE_INVERT)
        assert rc == R.RT_OK
        assert_same(out, want[perm], "permuted batch")
        for k in REF_COUNTERS:
            assert int(ctr[k]) == reps * int(f.ctr[1][k]), k
    finally:
        R.load().rt_dev_scene_free(s)


@pytest.mark.parametrize("option", ["inw_wide_walk", "inw_time_bins", "inw_sphere_records", "inw_compact_nodes",
                                    "inw_stackless", "inw_fused_cull", "inw_ri_grid"])
@pytest.mark.parametrize("name", ["glass600", "mixed300", "pile100", "cornell"])
def test_options_do_not_change_results(gpu, name, option):
    f = fx(name)
    with R.options(**{option: 0}):
        for invert in (0, 1):
            out, st = R.paths(f, f.rays, f.max_bounces, invert * R.RT_TRACE_INVERT)
            assert_same(out, f.out[invert], f"{name} {option}=0 invert {invert}")
            assert_ref_counters(stats_list(st), f.ctr[invert], f"{name} {option}=0 invert {invert}")


@pytest.mark.parametrize("device_build", [False, True])
def test_updated_scene_answers_as_the_new_frame(gpu, device_build):
    """rt_dev_scene_inw_update to glass600_b: with the caller's nodes, and with nodes = NULL and the
    boxes (the LBVH and the walk structures built on the device)."""
    a, b = fx("glass600"), fx("glass600_b")
    lib = R.load()
    s = dev_scene(a)
    try:
        rc = lib.rt_dev_scene_inw_update(s, R.fptr(b.geom), b.n, None if device_build else R.fptr(b.nodes),
                                         R.fptr(b.aabbs) if device_build else None, None, 0, None)
        assert rc == R.RT_OK
        for invert in (0, 1):
            rc, out, ctr = paths_async(s, b.rays, b.max_bounces, invert * R.RT_TRACE_INVERT)
            assert rc == R.RT_OK
            assert_same(out, b.out[invert], f"updated scene, invert {invert}")
            assert_ref_counters(ctr, b.ctr[invert], "updated scene")
    finally:
        lib.rt_dev_scene_free(s)


def _preset_scene(name):
    if name == "cam_random600":
        return R.make_scene(R.PRESET_INW01_RANDOM, 1234, 600, width=P.CAM_W, height=P.CAM_H, spp=P.SPP)
    return R.make_scene(R.PRESET_INW04_CORNELL, width=P.CAM_W, height=P.CAM_H, spp=P.SPP)


@pytest.mark.parametrize("name", P.CAM)
def test_a_frame_is_the_fold_of_its_path_queries(gpu, name):
    """The camera's own sample rays as path queries, folded on the host as End() folds them, are the
    GPU render's image and depth bit for bit, with the render's counts."""
    f = fx(name)
    sc = _preset_scene(name)
    assert np.array_equal(sc.geom, f.geom)
    sc.params.max_bounces = f.max_bounces
    rgba, depth, st = R.render(sc)
    inv = P.camera_invert(f.camera)
    out, pst = R.paths(f, f.rays, f.max_bounces, inv * R.RT_TRACE_INVERT)
    assert_same(out, f.out[inv], name)
    rgb, dep = P.fold(out, P.SPP)
    assert P.same(rgb, rgba[..., :3].reshape(-1, 3).copy())
    assert P.same(dep, depth.reshape(-1).copy())
    for k in ("segments", "shadow_queries", "stack_drops", "nan_drops"):
        assert pst[k] == st[k], k


@pytest.fixture(scope="module")
def ref_lib(tmp_path_factory):
    return P.build(tmp_path_factory.mktemp("path_ref"))


def test_far_origins_agree_with_the_reference_walk(gpu, ref_lib):
    """Query origins beyond the fused cull's bound (1000 from the world origin) send their whole path
    to the reference walks: the same bytes as a scene built without the wide walk, and as the oracle's loop."""
    f = fx("mixed300")
    rays = f.rays[:512].copy()
    length = np.linalg.norm(rays["d"].astype(np.float64), axis=1, keepdims=True)
    rays["o"] = (rays["o"] - rays["d"] / length * 3000.0).astype(np.float32)
    assert np.all(np.abs(rays["o"]).max(1) > 1000.0)
    out, _ = R.paths(f, rays, f.max_bounces)
    with R.options(inw_wide_walk=0):
        ref, _ = R.paths(f, rays, f.max_bounces)
    assert_same(out, ref, "far origins")
    assert 0.0 < (out["segments"] > 1).mean() < 1.0
    for invert in (0, 1):
        want, wctr = P.run(ref_lib, f, rays, invert)
        out, st = R.paths(f, rays, f.max_bounces, invert * R.RT_TRACE_INVERT)
        assert_same(out, want, f"far origins against the oracle, invert {invert}")
        assert_ref_counters(stats_list(st), wctr, f"far origins against the oracle, invert {invert}")


def test_invalid_samples(gpu):
    """sample >= spp: status 1, every other field 0, not counted; its wave's other lanes are unaffected."""
    f = fx("glass600")
    rays = f.rays[:256].copy()
    bad = np.zeros(256, bool)
    bad[[3, 64, 100, 101, 255]] = True
    rays["sample"][bad] = [16, 0xFFFFFFFF, 16, 0xFFFFFFFF, 17]
    s = dev_scene(f)
    try:
        rc, out, ctr = paths_async(s, rays, f.max_bounces, 0)
    finally:
        R.load().rt_dev_scene_free(s)
    assert rc == R.RT_OK
    assert np.all(out["status"][bad] == 1) and not out["status"][~bad].any()
    assert not out[bad].view(np.uint32).reshape(-1, 8)[:, :7].any()
    assert_same(out[~bad], f.out[0][:256][~bad], "neighbours of invalid samples")
    assert ctr[0] == f.out[0]["segments"][:256][~bad].sum()


def test_errors_on_a_device(gpu):
    lib = R.load()
    f = fx("one")
    s = dev_scene(f)
    try:
        assert paths_async(s, f.rays[:4], 8, R.RT_TRACE_ANY)[0] == R.RT_E_ARG   # a flag bit other than INVERT
        assert paths_async(s, f.rays[:4], 8, 4)[0] == R.RT_E_ARG
        assert paths_async(s, f.rays[:4], -1, 0)[0] == R.RT_E_ARG               # max_bounces < 0
        assert lib.rt_path_rays_async(s, None, 4, 8, 0, None, None, None) == R.RT_E_ARG
        assert lib.rt_path_rays_async(s, None, (1 << 31) + 1, 8, 0, None, None, None) == R.RT_E_ARG
        rc, out, ctr = paths_async(s, f.rays[:4], 8, 0, n_rays=0)              # nothing to do: nothing launched
        assert rc == R.RT_OK and np.all(out.view(np.uint8) == SENTINEL) and not ctr.any()
        assert lib.rt_path_rays_async(s, None, 0, 8, 0, None, None, None) == R.RT_OK
    finally:
        lib.rt_dev_scene_free(s)
    sc = R.make_scene(R.PRESET_IOW03_REF3, spp=1)
    s3 = lib.rt_dev_scene_iow03(R.fptr(sc.types), R.fptr(sc.records), sc.n, 1, -1)
    assert s3
    try:
        assert paths_async(s3, f.rays[:4], 8, 0)[0] == R.RT_E_UNSUPPORTED
    finally:
        lib.rt_dev_scene_free(s3)


def test_null_counters(gpu):
    f = fx("one")
    s = dev_scene(f)
    try:
        rc, out, ctr = paths_async(s, f.rays, f.max_bounces, 0, counters=False)
    finally:
        R.load().rt_dev_scene_free(s)
    assert rc == R.RT_OK and not ctr.any()
    assert_same(out, f.out[0], "NULL counters")


def test_kernel_resources(gpu):
    """The path kernel as loaded: the 40-float stacks of 256 lanes in LDS, and the registers and
    (no) scratch of DESIGN.md 5.9's table at three waves per SIMD."""
    table = {(False, False): 142, (False, True): 142, (True, False): 162, (True, True): 162}
    for (lights, fused), vgprs in table.items():
        info = R.paths_kernel_info(lights, fused)
        print("k_inw_paths", "lights" if lights else "inw01", "fused" if fused else "plain", info)
        assert info["lds_bytes"] == 40 * 256 * 4 and info["blocks_per_cu"] >= 1
        assert info["scratch_bytes"] == 0
        assert info["vgprs"] == vgprs
