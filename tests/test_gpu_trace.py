"""Batched closest-hit ray queries (rt_trace_rays_async / rt_trace_inw) on the GPU, bit for bit
against the fixtures tests/golden/trace_*.npz (the CPU oracle's closest-hit walk per query,
tests/trace_ref.c; tests/test_trace_ref.py recomputes them): t, id, normal, extra, the query count
and the dropped pushes, for both child orders, every scene option, ragged batch sizes, updated
scenes and the occlusion flag."""
import ctypes as C

import numpy as np
import pytest

import rt_amd as R
import trace_ref as T

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = 0xCD


class _Fx:
    """A fixture as a packed scene (what R.trace takes)."""

    def __init__(self, name):
        d = T.load_fixture(name)
        self.geom, self.nodes, self.aabbs, self.layout = d["geom"], d["nodes"], d["aabbs"], d["layout"]
        self.n = self.geom.shape[0]
        self.rays = d["rays"]
        self.hits = (d["hits0"], d["hits1"])
        self.drops = (int(d["ctr0"][2]), int(d["ctr1"][2]))


_cache = {}


def fx(name) -> _Fx:
    if name not in _cache:
        _cache[name] = _Fx(name)
    return _cache[name]


def dev_scene(f: _Fx):
    s = R.load().rt_dev_scene_inw(R.fptr(f.geom), f.n, f.layout, R.fptr(f.nodes), None, 0, 1, -1)
    assert s
    return s


def _wide_nodes(s) -> int:
    """rt_debug_wide_info: the nodes of the scene's wide tree (0: its queries take the reference walk)."""
    info = (C.c_uint32 * 8)()
    assert R.load().rt_debug_wide_info(s, info, None) == 0
    return int(info[0])


def trace_async(s, rays, flags, n_rays=None, cap=None):
    """rt_trace_rays_async on the current torch stream; the hit buffer (cap records) starts as
    SENTINEL bytes.  Returns (rc, hits (cap,), counters (6,))."""
    rays = np.ascontiguousarray(rays, R.RAY_DTYPE)
    n_rays = len(rays) if n_rays is None else n_rays
    cap = max(len(rays), 1) if cap is None else cap
    dev = torch.device("cuda")
    d_rays = torch.from_numpy(np.frombuffer(rays.tobytes() + bytes(32), np.uint8).copy()).to(dev)
    d_hits = torch.full((cap * 32,), SENTINEL, dtype=torch.uint8, device=dev)
    d_ctr = torch.zeros(6, dtype=torch.int64, device=dev)
    rc = R.load().rt_trace_rays_async(s, d_rays.data_ptr(), n_rays, flags, d_hits.data_ptr(), d_ctr.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, d_hits.cpu().numpy().view(R.HIT_DTYPE), d_ctr.cpu().numpy()


def assert_same(got, want, what):
    assert got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero((got.view(np.uint32).reshape(-1, 8) != want.view(np.uint32).reshape(-1, 8)).any(1))
        raise AssertionError(f"{what}: {len(bad)} of {len(got)} hits differ, first {bad[0]}: got {got[bad[0]]} "
                             f"want {want[bad[0]]}")


@pytest.mark.parametrize("invert", [0, 1])
@pytest.mark.parametrize("name", T.SCENES)
def test_parity_blocking_and_async(gpu, name, invert):
    f = fx(name)
    want = f.hits[invert]
    hits, st = R.trace(f, f.rays, invert * R.RT_TRACE_INVERT)
    assert_same(hits, want, f"{name} rt_trace_inw")
    assert st["segments"] == len(f.rays) and st["stack_drops"] == f.drops[invert]
    assert st["shadow_queries"] == 0 and st["nan_drops"] == 0
    s = dev_scene(f)
    try:
        rc, hits, ctr = trace_async(s, f.rays, invert * R.RT_TRACE_INVERT)
    finally:
        R.load().rt_dev_scene_free(s)
    assert rc == R.RT_OK
    assert_same(hits, want, f"{name} rt_trace_rays_async")
    assert ctr[0] == len(f.rays) and ctr[4] == f.drops[invert] and ctr[3] == 0 and ctr[5] == 0
    assert ctr[1] > 0 and ctr[2] > 0


def test_batch_sizes_and_untouched_tail(gpu):
    """Prefixes around the 64-query wave claim; hits past n_rays keep the sentinel."""
    f = fx("mixed700")
    s = dev_scene(f)
    try:
        for k in (0, 1, 63, 64, 65, 2047):
            rc, hits, ctr = trace_async(s, f.rays, R.RT_TRACE_INVERT, n_rays=k, cap=len(f.rays))
            assert rc == R.RT_OK, k
            assert_same(hits[:k], f.hits[1][:k], f"prefix {k}")
            assert np.all(hits[k:].view(np.uint8) == SENTINEL), k
            assert ctr[0] == k
    finally:
        R.load().rt_dev_scene_free(s)


@pytest.mark.parametrize("option", ["inw_wide_walk", "inw_time_bins", "inw_sphere_records", "inw_compact_nodes",
                                    "inw_stackless", "inw_fused_cull"])
@pytest.mark.parametrize("name", ["spheres1500", "mixed700", "dups300", "pile120", "shrunk06", "shrunk09"])
def test_options_do_not_change_results(gpu, name, option):
    f = fx(name)
    with R.options(**{option: 0}):
        for invert in (0, 1):
            hits, st = R.trace(f, f.rays, invert * R.RT_TRACE_INVERT)
            assert_same(hits, f.hits[invert], f"{name} {option}=0 invert {invert}")
            assert st["segments"] == len(f.rays) and st["stack_drops"] == f.drops[invert]


@pytest.mark.parametrize("device_build", [False, True])
def test_updated_scene_traces_as_the_new_frame(gpu, device_build):
    """rt_dev_scene_inw_update to spheres1500_b: with the caller's nodes, and with nodes = NULL and the
    boxes (the LBVH and the walk structures built on the device, node for node the host's)."""
    a, b = fx("spheres1500"), fx("spheres1500_b")
    lib = R.load()
    s = dev_scene(a)
    try:
        rc = lib.rt_dev_scene_inw_update(s, R.fptr(b.geom), b.n, None if device_build else R.fptr(b.nodes),
                                         R.fptr(b.aabbs) if device_build else None, None, 0, None)
        assert rc == R.RT_OK
        for invert in (0, 1):
            rc, hits, ctr = trace_async(s, b.rays, invert * R.RT_TRACE_INVERT)
            assert rc == R.RT_OK
            assert_same(hits, b.hits[invert], f"updated scene, invert {invert}")
            assert ctr[0] == len(b.rays) and ctr[4] == b.drops[invert]
    finally:
        lib.rt_dev_scene_free(s)


@pytest.mark.parametrize("device_build", [False, True])
def test_updated_scene_with_boxes_objects_stick_out_of(gpu, device_build):
    """mixed700 (the packers' boxes) updated to shrunk06, whose objects stick out of the caller's boxes
    (tests/test_trace_ref.py): with the caller's nodes, and with nodes = NULL and the shrunk boxes.  The
    answers follow the boxes given, for both child orders, and the scene no longer takes the wide
    walk (DESIGN.md §2 "Objects inside their leaf boxes")."""
    a, b = fx("mixed700"), fx("shrunk06")
    lib = R.load()
    s = dev_scene(a)
    try:
        rc, hits, _ = trace_async(s, a.rays, 0)
        assert rc == R.RT_OK
        assert_same(hits, a.hits[0], "mixed700 before the update")
        assert _wide_nodes(s) > 0
        rc = lib.rt_dev_scene_inw_update(s, R.fptr(b.geom), b.n, None if device_build else R.fptr(b.nodes),
                                         R.fptr(b.aabbs) if device_build else None, None, 0, None)
        assert rc == R.RT_OK
        for invert in (0, 1):
            rc, hits, ctr = trace_async(s, b.rays, invert * R.RT_TRACE_INVERT)
            assert rc == R.RT_OK
            assert_same(hits, b.hits[invert], f"updated to shrunk06, invert {invert}")
            assert ctr[0] == len(b.rays) and ctr[4] == b.drops[invert]
        assert _wide_nodes(s) == 0
    finally:
        lib.rt_dev_scene_free(s)


@pytest.mark.parametrize("name", ["spheres1500", "mixed700", "dups300", "pile120", "refset4"])
def test_any_hit(gpu, name):
    f = fx(name)
    for invert in (0, 1):
        want = f.hits[invert]
        hits, st = R.trace(f, f.rays, invert * R.RT_TRACE_INVERT | R.RT_TRACE_ANY)
        hit = want["id"] >= 0
        assert np.array_equal(hits["id"] >= 0, hit)
        assert np.all(hits["id"][hit] < f.n)
        assert np.all(want["t"][hit] <= hits["t"][hit]) and np.all(hits["t"][hit] < f.rays["tmax"][hit])
        assert np.array_equal(hits["t"][~hit].view(np.uint32), f.rays["tmax"][~hit].view(np.uint32))
        assert np.all(hits["id"][~hit] == -1)
        assert not hits["n"].any() and not hits["extra"].any() and not hits["pad"].any()
        assert st["segments"] == len(f.rays)


def test_limits_that_cannot_hit(gpu):
    """tmax <= 0 or NaN: a miss with t = tmax as passed."""
    f = fx("mixed700")
    rays = f.rays[:64].copy()
    rays["tmax"] = np.tile(np.array([0.0, -0.0, -1.0, np.nan], np.float32), 16)
    hits, st = R.trace(f, rays)
    assert np.array_equal(hits["t"].view(np.uint32), rays["tmax"].view(np.uint32))
    assert np.all(hits["id"] == -1) and not hits["n"].any() and not hits["extra"].any()
    assert st["segments"] == 64 and st["stack_drops"] == 0


@pytest.fixture(scope="module")
def ref_lib(tmp_path_factory):
    return T.build(tmp_path_factory.mktemp("trace_ref"))


def test_far_origins_agree_with_the_reference_walk(gpu, ref_lib):
    """Origins beyond the fused cull's bound (1000 from the world origin) take the reference walk:
    the same answers as a scene built without the wide walk, and as the oracle's walk."""
    f = fx("mixed700")
    rays = f.rays[:512].copy()
    length = np.linalg.norm(rays["d"].astype(np.float64), axis=1, keepdims=True)
    rays["o"] = (rays["o"] - rays["d"] / length * 3000.0).astype(np.float32)
    assert np.all(np.abs(rays["o"]).max(1) > 1000.0)
    hits, _ = R.trace(f, rays)
    with R.options(inw_wide_walk=0):
        ref, _ = R.trace(f, rays)
    assert_same(hits, ref, "far origins")
    assert 0.2 < (hits["id"] >= 0).mean() < 1.0
    for invert in (0, 1):
        want, ctr = T.run(ref_lib, f.geom, f.nodes, f.layout, rays, invert)
        hits, st = R.trace(f, rays, invert * R.RT_TRACE_INVERT)
        assert_same(hits, want, f"far origins against the oracle, invert {invert}")
        assert st["segments"] == len(rays) and st["stack_drops"] == int(ctr[2])


def test_errors_on_a_device(gpu):
    lib = R.load()
    f = fx("three")
    s = dev_scene(f)
    try:
        assert trace_async(s, f.rays[:4], 4)[0] == R.RT_E_ARG            # unknown flag bits
        assert lib.rt_trace_rays_async(s, None, 4, 0, None, None, None) == R.RT_E_ARG
        rc, hits, ctr = trace_async(s, f.rays[:4], 0, n_rays=0)            # nothing to do: nothing launched
        assert rc == R.RT_OK and np.all(hits.view(np.uint8) == SENTINEL) and not ctr.any()
        assert lib.rt_trace_rays_async(s, None, 0, 0, None, None, None) == R.RT_OK
    finally:
        lib.rt_dev_scene_free(s)
    sc = R.make_scene(R.PRESET_IOW03_REF3, spp=1)
    s3 = lib.rt_dev_scene_iow03(R.fptr(sc.types), R.fptr(sc.records), sc.n, 1, -1)
    assert s3
    try:
        assert trace_async(s3, f.rays[:4], 0)[0] == R.RT_E_UNSUPPORTED
    finally:
        lib.rt_dev_scene_free(s3)


def test_null_counters(gpu):
    f = fx("three")
    s = dev_scene(f)
    dev = torch.device("cuda")
    try:
        d_rays = torch.from_numpy(np.frombuffer(f.rays.tobytes(), np.uint8).copy()).to(dev)
        d_hits = torch.zeros(len(f.rays) * 32, dtype=torch.uint8, device=dev)
        rc = R.load().rt_trace_rays_async(s, d_rays.data_ptr(), len(f.rays), 0, d_hits.data_ptr(), None,
                                          torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        R.load().rt_dev_scene_free(s)
    assert rc == R.RT_OK
    assert_same(d_hits.cpu().numpy().view(R.HIT_DTYPE), f.hits[0], "NULL counters")


def test_kernel_resources(gpu):
    """The query kernel as loaded: no scratch, the 40-float stacks of 256 lanes in LDS."""
    for any_hit in (False, True):
        for fused in (False, True):
            info = R.trace_kernel_info(any_hit, fused)
            assert info["scratch_bytes"] == 0 and info["lds_bytes"] == 40 * 256 * 4
            assert 0 < info["vgprs"] <= 128 and info["blocks_per_cu"] >= 1
