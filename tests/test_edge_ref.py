"""The edge-case query fixtures (tests/golden/trace_edges_*.npz, paths_edges_*.npz) against their
reference, on the CPU: tests/trace_ref.c and tests/path_ref.c -- the oracle's own walk and sample
loop, which take any floats and any time ratio -- are rebuilt and recompute every fixture bit for bit,
and the fixtures hold what tests/test_gpu_query_edges.py relies on them for: every class of
degenerate ray (tests/edge_ref.py) with enough queries, hits and misses in the classes that can be
aimed, out-of-range time ratios whose answers differ from the clamped ratio's, bin-edge ratios that
hit moving objects, and scenes that do (spheres, mixed) or cannot (far) use the fused cull."""
import numpy as np
import pytest

import edge_ref as E
import path_ref as P
import rt_amd as R
import trace_ref as T


@pytest.fixture(scope="module")
def trace_lib(tmp_path_factory):
    return T.build(tmp_path_factory.mktemp("edge_trace_ref"))


@pytest.fixture(scope="module")
def path_lib(tmp_path_factory):
    return P.build(tmp_path_factory.mktemp("edge_path_ref"))


def bits(a):
    return a.view(np.uint32).reshape(len(a), -1)


@pytest.mark.parametrize("name", E.TRACE_SCENES)
def test_trace_fixture_recomputes_bit_for_bit(trace_lib, name):
    fx = E.load_trace(name)
    assert fx.geom.shape == (fx.n, 28) and fx.nodes.shape == (2 * fx.n - 1, 8) and fx.aabbs.shape == (fx.n, 6)
    assert fx.layout == 1 and fx.names == E.trace_class_names() and fx.cls.shape == fx.rays.shape
    for inv in (0, 1):
        hits, ctr = T.run(trace_lib, fx.geom, fx.nodes, fx.layout, fx.rays, inv)
        assert T.same_hits(hits, fx.hits[inv]), (name, inv)
        assert np.array_equal(ctr, fx.ctr[inv]), (name, inv)
        hits, ctr = T.run(trace_lib, fx.geom, fx.nodes, fx.layout, fx.rays_ratio, inv)
        assert T.same_hits(hits, fx.hits_ratio[inv]), (name, inv, "ratio")
        assert np.array_equal(ctr, fx.ctr_ratio[inv]), (name, inv, "ratio")


@pytest.mark.parametrize("name", E.PATH_SCENES)
def test_paths_fixture_recomputes_bit_for_bit(path_lib, name):
    fx = E.load_paths(name)
    assert fx.layout == (4 if name == "refset4" else 1) and fx.names == E.path_class_names()
    assert fx.spp == P.SPP and fx.max_bounces == E.MAX_BOUNCES
    for inv in (0, 1):
        out, ctr = P.run(path_lib, fx, fx.rays, inv)
        # x86 gives one NaN to every operation, so even the NaNs recompute bit for bit
        assert P.same(out, fx.out[inv]), (name, inv)
        assert np.array_equal(ctr, fx.ctr[inv]), (name, inv)


@pytest.mark.parametrize("name", E.TRACE_SCENES)
def test_trace_classes_are_present_and_not_vacuous(name):
    fx = E.load_trace(name)
    flags = {**E.CLASSES, **E.TRACE_CLASSES}
    assert np.all(fx.rays["tmax"] > 0)  # (queries with tmax <= 0 skip the walk: test_gpu_trace.py has those)
    for inv in (0, 1):
        hit = fx.hits[inv]["id"] >= 0
        for c, cname in enumerate(fx.names):
            m = fx.cls == c
            assert int(m.sum()) >= 16, (name, cname, int(m.sum()))
            if flags[cname]:
                frac = float(hit[m].mean())
                assert 0.25 <= frac <= 0.95, (name, inv, cname, frac)
        h = fx.hits[inv]
        assert np.all(h["id"][hit] < fx.n) and np.all(h["id"][~hit] == -1)
        assert np.array_equal(h["t"][~hit].view(np.uint32), fx.rays["tmax"][~hit].view(np.uint32))
        assert not h["n"][~hit].any() and not h["extra"][~hit].any() and not h["pad"].any()
    # the overflowing directions still hit cuboids (their slab test has no dot(d, d))
    if name != "spheres":
        for cname in ("dir_1e30", "dir_3e38"):
            assert (fx.hits[0]["id"][fx.cls == fx.names.index(cname)] >= 0).mean() >= 0.25, cname


@pytest.mark.parametrize("name", E.TRACE_SCENES)
def test_trace_classes_hold_what_their_names_say(name):
    fx = E.load_trace(name)
    r = fx.rays

    def of(cname):
        return r[fx.cls == fx.names.index(cname)]

    d = of("dir_octant")["d"]
    assert len({tuple(s) for s in np.sign(d)}) == 8 and np.all(d != 0)
    for cname, neg in (("dir_pzero", False), ("dir_nzero", True)):
        d = of(cname)["d"]
        zero = d == 0
        assert len({tuple(s) for s in np.sign(d)}) == 18 and np.all(zero.any(1))
        assert np.all(np.signbit(d[zero]) == neg)
    for cname, val in (("dir_sub149", 2.0 ** -149), ("dir_sub127", 2.0 ** -127), ("dir_min126", 2.0 ** -126),
                       ("dir_1e-30", np.float32(1e-30)), ("dir_1e30", np.float32(1e30)), ("dir_3e38", np.float32(3e38))):
        d = of(cname)["d"]
        at = np.abs(d) == np.float32(val)
        assert np.all(at.sum(1) == 1) and at.any(0).all(), cname  # one component, every axis in turn
        assert np.signbit(d[at]).any() and not np.signbit(d[at]).all(), cname
    assert np.all(np.isnan(of("dir_nan")["d"]).sum(1) == 1)
    d = of("dir_inf")["d"]
    assert np.all(np.isinf(d).sum(1) == 1) and (d == np.inf).any() and (d == -np.inf).any()
    d = of("dir_zero")["d"]
    assert np.all(d == 0) and len({tuple(s) for s in np.signbit(d)}) == 8
    q = of("org_plane")
    on = (q["o"][:, None, :] == fx.aabbs[None, :, 0:3]) | (q["o"][:, None, :] == fx.aabbs[None, :, 3:6])
    assert np.all((on.any(1) & (q["d"] == 0)).any(1))  # on some leaf-box plane of the axis the direction is zero on
    assert np.signbit(q["d"][q["d"] == 0]).any()
    q = of("org_centre")
    assert np.all((q["o"][:, None, :] == fx.geom[None, :, 0:3]).all(2).any(1)) and np.all(q["ratio"] == 1.0)
    q = of("org_900_tiny")
    tiny = np.isin(np.abs(q["d"]), np.array([1e-30, 2.0 ** -126, 2.0 ** -127], np.float32))
    assert np.all(tiny.sum(1) == 1)
    assert np.all(np.abs(q["o"][tiny]) > 900.0) and len(np.unique(np.abs(q["d"][tiny]))) == 3
    if name != "far":  # inside the fused cull's bound (far's scene has no fused cull)
        assert np.all(np.abs(q["o"]) <= 1000.0)
    assert np.all(np.abs(of("org_1e6")["o"]).max(1) > 5e5) and np.all(np.abs(of("org_1e30")["o"]).max(1) > 5e29)
    assert np.all(np.isnan(of("org_nan")["o"]).sum(1) == 1) and np.all(np.isinf(of("org_inf")["o"]).sum(1) == 1)
    o = np.abs(of("org_subnormal")["o"])
    assert np.all(((o > 0) & (o < np.float32(2.0 ** -126))).sum(1) == 1)
    assert np.all(of("tmax_inf")["tmax"] == np.inf) and np.all(of("tmax_fltmax")["tmax"] == np.finfo(np.float32).max)
    assert np.all(of("tmax_sub149")["tmax"] == np.float32(2.0 ** -149))
    assert np.all(of("tmax_min126")["tmax"] == np.float32(2.0 ** -126))
    for B in E.BINS:
        assert np.array_equal(np.unique(of(f"ratio_edge_B{B}")["ratio"]), np.unique(E.bin_edge_ratios(B)))
    assert np.all(of("ratio_below1")["ratio"] == np.nextafter(np.float32(1), np.float32(0)))
    z = of("ratio_negzero")["ratio"]
    assert np.all(z == 0) and np.all(np.signbit(z))
    # every other class keeps its ratio on k / 16, inside [0, 1]
    assert np.all((r["ratio"] >= 0) & (r["ratio"] <= 1))


@pytest.mark.parametrize("name", E.TRACE_SCENES)
def test_limits_around_a_hit(trace_lib, name):
    """tmax one ulp above a hit's t keeps the hit; tmax = t or one ulp below loses that object."""
    fx = E.load_trace(name)
    for cname, step in (("tmax_hit_below", -1), ("tmax_hit_exact", 0), ("tmax_hit_above", 1)):
        m = fx.cls == fx.names.index(cname)
        rays = fx.rays[m].copy()
        rays["tmax"] = 32000.0
        free, _ = T.run(trace_lib, fx.geom, fx.nodes, fx.layout, rays, 0)
        assert np.all(free["id"] >= 0)
        t = free["t"].view(np.int32) + step  # positive floats: the next float up or down
        assert np.array_equal(fx.rays["tmax"][m].view(np.int32), t), cname
        h = fx.hits[0][m]
        if step > 0:
            assert T.same_hits(h, free), cname
        else:
            assert np.all((h["id"] != free["id"]) | (h["t"] != free["t"])), cname


@pytest.mark.parametrize("name", E.TRACE_SCENES)
def test_out_of_range_ratios_differ_from_the_clamped_ratio(trace_lib, name):
    """What a walk that clamped the ratio (or walked the last time bin's tree) would get wrong: at
    least a quarter of these answers differ from the same ray's at ratio 0 (below 0) or 1 (above 1);
    a NaN ratio's from both."""
    fx = E.load_trace(name)
    rr = fx.rays_ratio
    assert np.array_equal(rr["ratio"].reshape(len(E.RATIOS_OUT), -1)[:, 0].view(np.uint32), E.RATIOS_OUT.view(np.uint32))
    assert not np.any((rr["ratio"] >= 0) & (rr["ratio"] <= 1))
    moving = (fx.geom[:, 15:18] != 0).any(1)
    assert moving.all()
    for inv in (0, 1):
        at = {}
        for v in (0.0, 1.0):
            rays = rr.copy()
            rays["ratio"] = v
            at[v], _ = T.run(trace_lib, fx.geom, fx.nodes, fx.layout, rays, inv)
        d0 = (bits(at[0.0]) != bits(fx.hits_ratio[inv])).any(1)
        d1 = (bits(at[1.0]) != bits(fx.hits_ratio[inv])).any(1)
        differs = np.where(np.isnan(rr["ratio"]), d0 & d1, np.where(rr["ratio"] < 0, d0, d1))
        assert differs.mean() >= 0.25, (name, inv, float(differs.mean()))
        # and both kinds of answer occur: objects found where only the extrapolated position has them
        hit = fx.hits_ratio[inv]["id"] >= 0
        assert int((hit & differs).sum()) >= 32 and int((~hit).sum()) >= 32, (name, inv)


@pytest.mark.parametrize("name", E.TRACE_SCENES)
def test_bin_edge_queries_hit_moving_objects(name):
    fx = E.load_trace(name)
    moving = (fx.geom[:, 15:18] != 0).any(1)
    for B in E.BINS:
        m = fx.cls == fx.names.index(f"ratio_edge_B{B}")
        ids = fx.hits[0]["id"][m]
        assert int(moving[ids[ids >= 0]].sum()) >= 8, (name, B)
        # around every edge b / B a query hits
        for r in np.unique(fx.rays["ratio"][m]):
            assert np.any(ids[fx.rays["ratio"][m] == r] >= 0), (name, B, float(r))


@pytest.mark.parametrize("name", E.TRACE_SCENES + ["paths:spheres", "paths:mixed", "paths:far"])
def test_scenes_take_the_walks_they_are_meant_for(name):
    """Host builds only (no device): spheres and mixed get a wide tree no reference push can overflow
    and culling boxes inside the fused cull's bound of 1000; far's boxes reach beyond it."""
    fx = E.load_paths(name[6:]) if name.startswith("paths:") else E.load_trace(name)
    info = R.inw_host_build(fx.nodes, fx.n)
    assert info["wide_nodes"] > 0 and info["dfs_high"] <= 40, info
    wbound = float(R.inw_host_dump(fx.nodes, fx.n)["wbound"])
    lo, hi = float(fx.aabbs[:, 0:3].min()), float(fx.aabbs[:, 3:6].max())
    if name.endswith("far"):
        assert wbound > 1000.0 and hi > 1000.0 and float(fx.aabbs[:, 3].min()) < 1000.0
    else:
        assert wbound <= 1000.0 and 900.0 < max(-lo, hi) <= 1000.0
    if name.endswith("spheres"):
        g = fx.geom
        assert fx.n == 300 and np.all(g[:, 12] == g[:, 13]) and np.all(g[:, 12] == g[:, 14])
    else:
        assert fx.n == 200 and np.any(fx.geom[:, 12] != fx.geom[:, 13])


def _leaf_entry(box, o, d):
    """TestIntersectAABB's entry t of rays (o, d) into their own boxes, in float32 as the walks form it."""
    with np.errstate(all="ignore"):
        inv = np.float32(1.0) / d
        a, b = (box[:, 0:3] - o) * inv, (box[:, 3:6] - o) * inv
    return np.minimum(a, b).max(1)


@pytest.mark.parametrize("name", E.TRACE_SCENES + ["paths:spheres", "paths:mixed", "paths:far"])
def test_far_origins_put_t_below_the_box_entry(name):
    """What org_far is for: from thousands of units away the object test's t (its quadratic cancels)
    falls below the hit object's own leaf-box entry by more than the wide walk's margin
    t * 1.0001 + 1e-3, for a good part of the hits -- all inside a path's limit of 32000."""
    paths = name.startswith("paths:")
    fx = E.load_paths(name[6:]) if paths else E.load_trace(name)
    m = fx.cls == fx.names.index("org_far")
    r = fx.rays[m]
    away = np.linalg.norm(r["o"].astype(np.float64) - np.median(fx.geom[:, 0:3], axis=0), axis=1)
    assert away.min() > 2500.0 and away.max() < 32000.0
    if paths:
        for inv in (0, 1):
            assert (fx.out[inv]["segments"][m] > 1).mean() >= 0.25, (name, inv)
        return
    h = fx.hits[0][m]
    hit = h["id"] >= 0
    te = _leaf_entry(fx.aabbs[h["id"][hit]], r["o"][hit], r["d"][hit])
    below = h["t"][hit] * np.float32(1.0001) + np.float32(1e-3) < te
    assert hit.mean() >= 0.25 and below.mean() >= 0.2, (name, float(hit.mean()), float(below.mean()))


@pytest.mark.parametrize("name", E.PATH_SCENES)
def test_path_classes_are_present_and_not_vacuous(name):
    fx = E.load_paths(name)
    r = fx.rays
    bad = fx.cls == fx.names.index("bad_sample")
    assert int(bad.sum()) >= 8 and np.all(r["sample"][bad] >= fx.spp) and np.all(r["sample"][~bad] < fx.spp)
    assert set(r["sample"][~bad]) == set(range(fx.spp))  # cycles 0..spp-1, spp-1 included
    for c, cname in enumerate(fx.names):
        assert int((fx.cls == c).sum()) >= 16, (name, cname)
    for inv in (0, 1):
        o = fx.out[inv]
        assert np.all(o["status"][bad] == 1) and not o["status"][~bad].any()
        assert not bits(o[bad])[:, :7].any()
        assert int(o["segments"].sum()) == int(fx.ctr[inv][0]) and np.all(o["segments"][~bad] >= 1)
        assert int(o["nans"].sum()) == int(fx.ctr[inv][5]) > 0
        assert np.isnan(o["rgb"]).any() and (o["segments"] > 1).mean() > 0.1
        if name != "refset4":  # the aimed classes bounce (hit) and end at once (miss) side by side
            for cname, aimed in E.CLASSES.items():
                if aimed and cname != "org_1e6":  # (a path's limit is 32000: from 1e6 away every ray misses)
                    m = fx.cls == fx.names.index(cname)
                    assert 0 < (o["segments"][m] > 1).sum() < m.sum(), (name, inv, cname)
    if name == "refset4":
        assert fx.n_lights > 0 and int(fx.ctr[0][3]) > 0  # shadow rays
