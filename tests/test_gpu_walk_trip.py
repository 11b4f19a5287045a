"""The wide walk's trip (csrc/rt_inw_walk.hpp: inw_traverse_wide) on the GPU, bit for bit against
the CPU oracle: the walk-trip fixtures (tests/golden/trace_walk_*.npz; what each holds is asserted
on the CPU by tests/test_walk_trip_ref.py) through both ray-query entry points and both child
orders, partial waves, the options that change the walk's inputs, and two small frames through
the render kernels (k_inw_pm / k_inw_sm and the shadow walks)."""
import numpy as np
import pytest

import rt_amd as R
import trace_ref as T
import walk_trip_cases as W
from oracle import oracle as O
from test_gpu_trace import assert_same, dev_scene, fx, trace_async

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.mark.parametrize("invert", [0, 1])
@pytest.mark.parametrize("name", W.FIXTURES)
def test_fixture_both_entry_points(gpu, name, invert):
    f = fx(name)
    want = f.hits[invert]
    assert f.drops[invert] == 0
    hits, st = R.trace(f, f.rays, invert * R.RT_TRACE_INVERT)
    assert_same(hits, want, f"{name} rt_trace_inw")
    assert st["segments"] == len(f.rays) and st["stack_drops"] == 0 and st["nan_drops"] == 0
    s = dev_scene(f)
    try:
        rc, hits, ctr = trace_async(s, f.rays, invert * R.RT_TRACE_INVERT)
    finally:
        R.load().rt_dev_scene_free(s)
    assert rc == R.RT_OK
    assert_same(hits, want, f"{name} rt_trace_rays_async")
    assert ctr[0] == len(f.rays) and ctr[4] == 0 and ctr[1] > 0 and ctr[2] > 0


@pytest.mark.parametrize("name", ["walk_chain", "walk_moving", "walk_pile", "walk_three", "walk_one"])
def test_partial_waves(gpu, name):
    """1, 63, 64 and 65 queries: the last wave's other lanes walk nothing; windows that start inside
    a fixture wave put other lanes beside the overflowing and the refused ones."""
    f = fx(name)
    s = dev_scene(f)
    try:
        for invert in (0, 1):
            for lo, k in ((0, 1), (0, 63), (0, 64), (0, 65), (15, 1), (9, 65), (130, 63)):
                rays = f.rays[lo:lo + k]
                rc, hits, ctr = trace_async(s, rays, invert * R.RT_TRACE_INVERT)
                assert rc == R.RT_OK
                assert_same(hits, f.hits[invert][lo:lo + k], f"{name} [{lo}:{lo + k}] invert {invert}")
                assert ctr[0] == k and ctr[4] == 0
    finally:
        R.load().rt_dev_scene_free(s)


@pytest.mark.parametrize("option", ["inw_sphere_records", "inw_fused_cull", "inw_time_bins", "inw_compact_nodes"])
@pytest.mark.parametrize("name", ["walk_face", "walk_moving", "walk_chain", "walk_pile"])
def test_options_do_not_change_results(gpu, name, option):
    """inw_sphere_records 0 and 1 on walk_face, an all-sphere scene with sphere records (asserted on
    the CPU): its hits at the leaf-box entry go through the sphere-record leaf test and through the
    full-record one; the unfused cull on the rays the fused one refuses; one tree instead of the
    two time-bin trees."""
    f = fx(name)
    with R.options(**{option: 0}):
        for invert in (0, 1):
            hits, st = R.trace(f, f.rays, invert * R.RT_TRACE_INVERT)
            assert_same(hits, f.hits[invert], f"{name} {option}=0 invert {invert}")
            assert st["segments"] == len(f.rays) and st["stack_drops"] == 0


def test_overflowing_lanes_fall_back(gpu):
    """walk_chain's rays along the row overflow the walk's stack and are answered by the reference
    walk: the same hits as a scene without the wide walk.  The node visits say so directly: each
    lane's count is the reference walk's plus four per node step the wide walk took before a push
    went past cap, and the CPU model (W.walk_model over the host-built nodes) gives those steps."""
    f = fx("walk_chain")
    d = T.load_fixture("walk_chain")
    row = np.flatnonzero(np.arange(len(f.rays)) % 64 < 16)
    wn, links, _ = W.wide_nodes(d)
    steps = 0
    for q in row:
        over, _, n = W.walk_model(wn, links, 1, f.rays["o"][q], f.rays["d"][q], f.rays["tmax"][q])
        assert over
        steps += n
    hits, st = R.trace(f, f.rays[row])
    with R.options(inw_wide_walk=0):
        ref, st_ref = R.trace(f, f.rays[row])
    assert_same(hits, ref, "row rays")
    assert_same(hits, f.hits[0][row], "row rays against the oracle")
    print("node visits", st["node_visits"], "reference walk", st_ref["node_visits"], "wide steps", steps)
    assert st["node_visits"] == st_ref["node_visits"] + 4 * steps
    # a pending leaf of the abandoned walk is still tested: at most one per lane on top of the reference's
    assert st_ref["prim_tests"] <= st["prim_tests"] <= st_ref["prim_tests"] + len(row)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


@pytest.mark.parametrize("case", ["inw01_random_300", "c5_cornell"])
def test_small_frames_match_the_oracle(gpu, case):
    """k_inw_pm (inw_order 1, pixel-major) on 300 moving spheres (64 x 64, 8 spp) and k_inw_sm
    (inw_order 2, sample-major) on the C5 preset with its shadow walks (32 x 32, 4 spp): colour,
    depth and the ray-level counters."""
    if case == "inw01_random_300":
        sc, order = R.make_scene(R.PRESET_INW01_RANDOM, 1234, 300, width=64, height=64, spp=8), 1
    else:
        sc, order = R.make_scene(R.PRESET_INW04_CORNELL, 7, 0, width=32, height=32, spp=4), 2
    with R.options(inw_order=order):
        rgba, depth, st = R.render(sc, sc.params)
    orgba, odepth, ost = O.render(sc, sc.params)
    assert _same(rgba, orgba), "colour differs from the oracle"
    assert _same(depth, odepth), "depth differs from the oracle"
    for k in ("segments", "stack_drops", "nan_drops", "shadow_queries"):
        assert st[k] == ost[k], (k, st[k], ost[k])
    assert st["segments"] > 64 * 64
