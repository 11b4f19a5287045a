"""Ray and path queries with degenerate rays on the GPU, against the fixtures
tests/golden/trace_edges_*.npz and paths_edges_*.npz (the CPU oracle's answers; tests/test_edge_ref.py
recomputes them): directions with +-0.0, subnormal, tiny, huge, NaN and infinite components, origins
on leaf-box planes, on object centres, far out, NaN, infinite and subnormal, limits of +inf, FLT_MAX,
the smallest floats and one ulp around a hit, time ratios one ulp around every time-bin edge, and
time ratios outside [0, 1], which the trace kernel answers with the reference walk.

Comparison: bit for bit on every field and counter, except that a float field holding a NaN equals
any NaN (edge_ref.canon: the CPU's and the GPU's default NaNs differ in sign); numbers stay exact."""
import numpy as np
import pytest

import edge_ref as E
import rt_amd as R
from test_gpu_paths import REF_COUNTERS, paths_async, stats_list
from test_gpu_paths import dev_scene as paths_scene
from test_gpu_trace import _wide_nodes, dev_scene, trace_async

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

_cache = {}


def tfx(name):
    if ("t", name) not in _cache:
        _cache["t", name] = E.load_trace(name)
    return _cache["t", name]


def pfx(name):
    if ("p", name) not in _cache:
        _cache["p", name] = E.load_paths(name)
    return _cache["p", name]


def assert_same(got, want, canon, cls, names, what):
    assert got.shape == want.shape, what
    msg = E.first_difference(canon(got), canon(want), cls, names)
    if msg:
        raise AssertionError(f"{what}: {msg}")


def assert_hits(got, f, invert, what):
    assert_same(got, f.hits[invert], E.canon_hits, f.cls, f.names, what)


def assert_ratio_hits(got, f, invert, what):
    cls = np.repeat(np.arange(len(E.RATIOS_OUT)), len(f.rays_ratio) // len(E.RATIOS_OUT))
    assert_same(got, f.hits_ratio[invert], E.canon_hits, cls, [f"ratio {float(r)!r}" for r in E.RATIOS_OUT], what)


def assert_out(got, f, invert, what):
    assert_same(got, f.out[invert], E.canon_out, f.cls, f.names, what)


@pytest.mark.parametrize("invert", [0, 1])
@pytest.mark.parametrize("name", E.TRACE_SCENES)
def test_trace_blocking_and_async(gpu, name, invert):
    f = tfx(name)
    hits, st = R.trace(f, f.rays, invert * R.RT_TRACE_INVERT)
    assert_hits(hits, f, invert, f"{name} rt_trace_inw")
    assert st["segments"] == len(f.rays) and st["stack_drops"] == int(f.ctr[invert][2])
    assert st["shadow_queries"] == 0 and st["nan_drops"] == 0
    s = dev_scene(f)
    try:
        # the wide walk is what answers the finite classes; the host launches the fused-cull instance
        # for spheres and mixed and must not for far (boxes beyond 1000); sphere records in spheres
        assert _wide_nodes(s) > 0
        assert R.load().rt_debug_query_fused(s) == (0 if name == "far" else 1)
        assert (R.walk_dump(s, R.RT_WALK_SPH)[1][0] > 0) == (name == "spheres")
        rc, hits, ctr = trace_async(s, f.rays, invert * R.RT_TRACE_INVERT)
    finally:
        R.load().rt_dev_scene_free(s)
    assert rc == R.RT_OK
    assert_hits(hits, f, invert, f"{name} rt_trace_rays_async")
    assert ctr[0] == len(f.rays) and ctr[4] == int(f.ctr[invert][2]) and ctr[3] == 0 and ctr[5] == 0
    assert ctr[1] > 0 and ctr[2] > 0


OPTIONS = [("inw_wide_walk", 0), ("inw_sphere_records", 0), ("inw_compact_nodes", 0), ("inw_fused_cull", 0),
           ("inw_stackless", 0), ("inw_walk_bins", 0), ("inw_time_bins", 0), ("inw_time_bins", 3),
           ("inw_time_bins", 7), ("inw_time_bins", 16)]


@pytest.mark.parametrize("option", OPTIONS, ids=[f"{k}={v}" for k, v in OPTIONS])
@pytest.mark.parametrize("name", E.TRACE_SCENES)
def test_trace_options_do_not_change_results(gpu, name, option):
    """Each option alone; inw_time_bins = 3, 7, 16 put the ratio_edge_B* queries one ulp either side of a
    boundary between two time-bin trees."""
    f = tfx(name)
    with R.options(**{option[0]: option[1]}):
        for invert in (0, 1):
            hits, st = R.trace(f, f.rays, invert * R.RT_TRACE_INVERT)
            assert_hits(hits, f, invert, f"{name} {option[0]}={option[1]} invert {invert}")
            assert st["segments"] == len(f.rays) and st["stack_drops"] == int(f.ctr[invert][2])


@pytest.mark.parametrize("name", E.TRACE_SCENES)
def test_any_hit(gpu, name):
    f = tfx(name)
    for invert in (0, 1):
        want = f.hits[invert]
        hits, st = R.trace(f, f.rays, invert * R.RT_TRACE_INVERT | R.RT_TRACE_ANY)
        hit = want["id"] >= 0
        bad = np.flatnonzero((hits["id"] >= 0) != hit)
        assert not len(bad), (name, invert, f.names[f.cls[bad[0]]], int(bad[0]), hits[bad[0]], want[bad[0]])
        assert np.all(hits["id"][hit] < f.n)
        assert np.all(want["t"][hit] <= hits["t"][hit]) and np.all(hits["t"][hit] < f.rays["tmax"][hit])
        assert np.array_equal(hits["t"][~hit].view(np.uint32), f.rays["tmax"][~hit].view(np.uint32))
        assert np.all(hits["id"][~hit] == -1)
        assert not hits["n"].any() and not hits["extra"].any() and not hits["pad"].any()
        assert st["segments"] == len(f.rays)


@pytest.mark.parametrize("bins", [None, 16])
@pytest.mark.parametrize("name", E.TRACE_SCENES)
def test_ratios_outside_0_1_take_the_reference_walk(gpu, name, bins):
    """-1e-3 ... -inf, 1 + ulp ... +inf and NaN: the shader's position - delta * (1 - ratio) for any
    ratio, never a time-bin tree (whose index such a ratio does not give)."""
    f = tfx(name)
    with R.options(**({} if bins is None else {"inw_time_bins": bins})):
        for invert in (0, 1):
            hits, st = R.trace(f, f.rays_ratio, invert * R.RT_TRACE_INVERT)
            assert_ratio_hits(hits, f, invert, f"{name} bins {bins} rt_trace_inw invert {invert}")
            assert st["segments"] == len(f.rays_ratio) and st["stack_drops"] == int(f.ctr_ratio[invert][2])
        s = dev_scene(f)
        try:
            assert _wide_nodes(s) > 0
            for invert in (0, 1):
                rc, hits, ctr = trace_async(s, f.rays_ratio, invert * R.RT_TRACE_INVERT)
                assert rc == R.RT_OK
                assert_ratio_hits(hits, f, invert, f"{name} bins {bins} rt_trace_rays_async invert {invert}")
                assert ctr[0] == len(f.rays_ratio) and ctr[4] == int(f.ctr_ratio[invert][2])
                # the same rays as occlusion queries
                rc, anyh, _ = trace_async(s, f.rays_ratio, invert * R.RT_TRACE_INVERT | R.RT_TRACE_ANY)
                assert rc == R.RT_OK
                assert np.array_equal(anyh["id"] >= 0, f.hits_ratio[invert]["id"] >= 0)
        finally:
            R.load().rt_dev_scene_free(s)


def _ref_counters(ctr, want, what):
    for k in REF_COUNTERS:
        assert int(ctr[k]) == int(want[k]), (what, k, int(ctr[k]), int(want[k]))


@pytest.mark.parametrize("invert", [0, 1])
@pytest.mark.parametrize("name", E.PATH_SCENES)
def test_paths_blocking_and_async(gpu, name, invert):
    f = pfx(name)
    bad = f.cls == f.names.index("bad_sample")
    out, st = R.paths(f, f.rays, f.max_bounces, invert * R.RT_TRACE_INVERT)
    assert_out(out, f, invert, f"{name} rt_path_inw")
    _ref_counters(stats_list(st), f.ctr[invert], f"{name} rt_path_inw")
    assert np.all(out["status"][bad] == 1) and not out["status"][~bad].any()
    s = paths_scene(f)
    try:
        assert _wide_nodes(s) > 0
        assert R.load().rt_debug_query_fused(s) == (0 if name == "far" else 1)
        rc, out, ctr = paths_async(s, f.rays, f.max_bounces, invert * R.RT_TRACE_INVERT)
    finally:
        R.load().rt_dev_scene_free(s)
    assert rc == R.RT_OK
    assert_out(out, f, invert, f"{name} rt_path_rays_async")
    _ref_counters(ctr, f.ctr[invert], f"{name} rt_path_rays_async")
    assert np.all(out["status"][bad] == 1) and not out["status"][~bad].any()
    assert not out[bad].view(np.uint32).reshape(-1, 8)[:, :7].any()
    assert ctr[1] > 0 and ctr[2] > 0


@pytest.mark.parametrize("option", ["inw_wide_walk", "inw_fused_cull"])
@pytest.mark.parametrize("name", E.PATH_SCENES)
def test_paths_options_do_not_change_results(gpu, name, option):
    """The reference walks only, and the wide walk without the fused cull: there the org_far paths
    (origins 3000 to 20000 away, t below the hits' box entries) would take the wide walk if the path
    kernel tested a query's origin in its fused instance only."""
    f = pfx(name)
    with R.options(**{option: 0}):
        s = paths_scene(f)
        try:
            assert R.load().rt_debug_query_fused(s) == 0  # (the fused cull is the wide walk's)
            assert (_wide_nodes(s) > 0) == (option != "inw_wide_walk")
        finally:
            R.load().rt_dev_scene_free(s)
        for invert in (0, 1):
            out, st = R.paths(f, f.rays, f.max_bounces, invert * R.RT_TRACE_INVERT)
            assert_out(out, f, invert, f"{name} {option}=0 invert {invert}")
            _ref_counters(stats_list(st), f.ctr[invert], f"{name} {option}=0 invert {invert}")
