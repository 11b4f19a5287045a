"""The IOW-03 ray-query fixtures (tests/golden/trace_iow_*.npz) against their reference, on the CPU:
tests/trace_iow_ref.c -- the oracle's own launch_ray() per query, cross-checked against a restated
loop for (t, id) -- is rebuilt and recomputes every fixture bit for bit, and the fixtures exercise
what the GPU tests rely on them for: hits and misses in every scene, every ray kind, exact ties going
to the lowest index (dups, touch) and limits that cut off a real hit."""
import numpy as np
import pytest

import rt_amd as R
import trace_iow_ref as T


@pytest.fixture(scope="module")
def ref_lib(tmp_path_factory):
    return T.build(tmp_path_factory.mktemp("trace_iow_ref"))


@pytest.mark.parametrize("name", T.SCENES)
def test_fixture_recomputes_bit_for_bit(ref_lib, name):
    fx = T.load_fixture(name)
    n = len(fx["types"])
    assert fx["records"].shape == (n, 24) and fx["rays"].shape == (2048,)
    hits = T.run(ref_lib, fx["types"], fx["records"], fx["rays"])
    assert T.same_hits(hits, fx["hits"]), name


@pytest.mark.parametrize("name", T.SCENES)
def test_uncut_queries_hit_the_same_object(ref_lib, name):
    """A query written with tmax drawn around a real hit's t: with tmax = 32000 it hits cut_id; with
    its own tmax it hits cut_id or, the limit below the hit's t, nothing."""
    fx = T.load_fixture(name)
    cut = fx["cut_id"] >= 0
    assert cut.sum() >= 200
    rays = fx["rays"][cut].copy()
    rays["tmax"] = np.float32(32000.0)
    uncut = T.run(ref_lib, fx["types"], fx["records"], rays)
    assert np.array_equal(uncut["id"], fx["cut_id"][cut])
    got = fx["hits"][cut]
    kept = got["id"] >= 0
    assert 20 <= kept.sum() <= cut.sum() - 20  # both sides of the limit
    assert np.array_equal(got["id"][kept], uncut["id"][kept])
    assert np.array_equal(got["t"][kept].view(np.uint32), uncut["t"][kept].view(np.uint32))
    assert np.all(fx["rays"]["tmax"][cut][~kept] <= uncut["t"][~kept])


@pytest.mark.parametrize("name", T.SCENES)
def test_fixture_hits_are_well_formed(name):
    fx = T.load_fixture(name)
    rays, h = fx["rays"], fx["hits"]
    hit = h["id"] >= 0
    assert 0.10 <= float(hit.mean()) <= 0.90, name
    assert np.all(h["id"][hit] < len(fx["types"])) and np.all(h["id"][~hit] == -1)
    assert np.all(h["t"][hit] < rays["tmax"][hit]) and np.all(h["t"][hit] > 0)
    assert np.array_equal(h["t"][~hit].view(np.uint32), rays["tmax"][~hit].view(np.uint32))
    assert not h["n"][~hit].any() and not h["extra"][~hit].any() and not h["pad"].any()
    # a hit's extra is its object's record float 20, its normal is normalised
    assert np.array_equal(h["extra"][hit].view(np.uint32), fx["records"][h["id"][hit], 20].view(np.uint32))
    assert np.allclose(np.linalg.norm(h["n"][hit].astype(np.float64), axis=1), 1.0, atol=1e-5)


@pytest.mark.parametrize("name", T.SCENES)
def test_ray_kinds_present(name):
    fx = T.load_fixture(name)
    r, h = fx["rays"], fx["hits"]
    d2 = (r["d"].astype(np.float64) ** 2).sum(1)
    assert np.all((r["d"][3::8] == 0).sum(1) == 2)                    # axis-parallel
    k4 = d2[4::8]
    for lo, hi in ((0.24, 0.26), (3.9, 4.1), (0.998, 0.9985), (0.9975, 0.998), (1.0015, 1.002), (1.002, 1.0025)):
        assert ((k4 > lo) & (k4 < hi)).sum() >= 30, (name, lo, hi)   # lengths 0.5, 2, the band's four sides
    k5 = r[5::8]
    assert (np.abs(k5["d"]).sum(1) == 0).sum() >= 30 and np.isnan(k5["d"]).any(1).sum() >= 30
    for v in (np.inf, 0.0, -1.0, 32000.0):
        assert (k5["tmax"] == np.float32(v)).sum() >= 30, (name, v)
    assert np.isnan(k5["tmax"]).sum() >= 30
    assert np.all(h["id"][5::8][~(k5["tmax"] > 0) | ~(d2[5::8] > 0)] == -1)  # ... all of them misses
    assert len(np.unique(r["ratio"].view(np.uint32))) > 2000           # random bits
    assert (h["id"][1::8] >= 0).mean() > 0.9                           # origins inside objects hit them


def test_scene_sizes():
    """The node counts that decide the kernel's path: LDS (<= 240), global, one node, no BVH."""
    want = {"final": (486, 235), "final2": (972, 530), "ref3": (3, 1), "one": (1, 0)}
    for name in T.SCENES:
        fx = T.load_fixture(name)
        n = len(fx["types"])
        nodes = R.iow_host_build(fx["types"], fx["records"], n)["wide_nodes"]
        if name in want:
            assert (n, nodes) == want[name], name
        if name == "shells":
            assert 0 < nodes <= 240 and fx["ovf"].sum() == 256
            assert np.all(fx["rays"]["o"][fx["ovf"]] == fx["records"][0, 0:3])
        elif name == "chain":
            assert 0 < nodes <= 240 and fx["ovf"].sum() == 256
            r = fx["rays"][fx["ovf"]]
            assert np.all(r["d"] == (1, 0, 0)) and np.all(r["o"][:, 0] == 0) and np.all(np.isinf(r["tmax"])) and np.all(fx["hits"]["id"][fx["ovf"]] == 0)
        else:
            assert not fx["ovf"].any()


def test_rot_has_rotated_unequal_objects():
    fx = T.load_fixture("rot")
    rec = fx["records"]
    eye = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], np.float32)
    assert np.all(np.any(rec[:, 3:12] != eye, axis=1))
    assert np.all(rec[:, 12:15].max(1) > rec[:, 12:15].min(1))
    assert set(np.unique(fx["types"])) == {1.0, 2.0}


def test_dups_ties_go_to_the_lowest_index():
    fx = T.load_fixture("dups")
    rec, h = fx["records"], fx["hits"]
    assert np.array_equal(rec[:100], rec[100:200]) and np.array_equal(rec[:100], rec[200:])
    hit = h["id"] >= 0
    assert hit.sum() > 1000 and np.all(h["id"][hit] < 100)


def test_touch_has_cross_object_ties(ref_lib):
    """Unit cuboids at unit spacing share faces: for some queries the winner's t is also the t of a
    neighbour with a higher index (dropping the winner leaves t unchanged)."""
    fx = T.load_fixture("touch")
    h = fx["hits"]
    pick = np.flatnonzero(h["id"] >= 0)[:400]
    ties = 0
    for q in pick:
        types = fx["types"].copy()
        types[h["id"][q]] = 0.0  # an object of no type is never hit (t = -1)
        other = T.run(ref_lib, types, fx["records"], fx["rays"][q:q + 1])
        if other["id"][0] >= 0 and other["t"][0] == h["t"][q]:
            assert other["id"][0] > h["id"][q]
            ties += 1
    assert ties >= 10, ties
