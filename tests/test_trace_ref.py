"""The ray-query fixtures (tests/golden/trace_*.npz) against their reference, on the CPU:
tests/trace_ref.c -- the oracle's own closest-hit walk per query -- is rebuilt and recomputes
every fixture bit for bit, and the fixtures exercise what the GPU tests rely on them for: hits
and misses in every scene, exact ties decided by the child order (dups300), and pushes the full
40-float stack drops (pile120)."""
import numpy as np
import pytest

import trace_ref as T


@pytest.fixture(scope="module")
def ref_lib(tmp_path_factory):
    return T.build(tmp_path_factory.mktemp("trace_ref"))


@pytest.mark.parametrize("name", T.SCENES)
def test_fixture_recomputes_bit_for_bit(ref_lib, name):
    fx = T.load_fixture(name)
    n = fx["geom"].shape[0]
    assert fx["geom"].shape == (n, 28) and fx["nodes"].shape == (2 * n - 1, 8) and fx["aabbs"].shape == (n, 6)
    assert fx["rays"].shape == (2048,) and fx["layout"] in (1, 4)
    for inv in (0, 1):
        hits, ctr = T.run(ref_lib, fx["geom"], fx["nodes"], fx["layout"], fx["rays"], inv)
        assert T.same_hits(hits, fx[f"hits{inv}"]), (name, inv)
        assert np.array_equal(ctr, fx[f"ctr{inv}"]), (name, inv)


@pytest.mark.parametrize("name", T.SCENES)
def test_fixture_hits_are_well_formed(name):
    fx = T.load_fixture(name)
    rays = fx["rays"]
    assert np.all(rays["tmax"] > 0)  # (queries with tmax <= 0 skip the walk: their drops are not the fixture's)
    for inv in (0, 1):
        h = fx[f"hits{inv}"]
        hit = h["id"] >= 0
        frac = float(hit.mean())
        assert 0.2 <= frac <= 0.95, (name, inv, frac)
        assert np.all(h["id"][hit] < fx["geom"].shape[0]) and np.all(h["id"][~hit] == -1)
        assert np.all(h["t"][hit] < rays["tmax"][hit]) and np.all(h["t"][hit] > 0)
        assert np.array_equal(h["t"][~hit].view(np.uint32), rays["tmax"][~hit].view(np.uint32))
        assert not h["n"][~hit].any() and not h["extra"][~hit].any() and not h["pad"].any()
        # a hit's extra is its object's record float 19
        assert np.array_equal(h["extra"][hit].view(np.uint32), fx["geom"][h["id"][hit], 19].view(np.uint32))
    # the child order changes no hit mask unless a push dropped
    if not fx["ctr0"][2] and not fx["ctr1"][2]:
        assert np.array_equal(fx["hits0"]["id"] >= 0, fx["hits1"]["id"] >= 0)
        assert np.array_equal(fx["hits0"]["t"].view(np.uint32), fx["hits1"]["t"].view(np.uint32))


def test_ray_kinds_present():
    """Axis-aligned directions (two zero components), un-normalised ones and limited rays."""
    r = T.load_fixture("mixed700")["rays"]
    assert np.all((r["d"][4::8] == 0).sum(1) == 2)
    length = np.linalg.norm(r["d"][5::8].astype(np.float64), axis=1)
    assert length.min() < 0.1 and length.max() > 10.0
    assert np.all(r["tmax"][3::8] < 32000.0) and np.all(r["tmax"][2::8] == 32000.0)
    assert len(np.unique(r["ratio"])) == 17 and r["ratio"].min() == 0.0 and r["ratio"].max() == 1.0


def test_dups300_ties_follow_child_order():
    fx = T.load_fixture("dups300")
    h0, h1 = fx["hits0"], fx["hits1"]
    assert np.array_equal(h0["t"].view(np.uint32), h1["t"].view(np.uint32))
    differs = h0["id"] != h1["id"]
    assert int(differs.sum()) >= 500
    assert np.all(np.abs(h0["id"][differs] - h1["id"][differs]) == 150)  # the same sphere's other copy


def test_pile120_overflows_the_stack():
    fx = T.load_fixture("pile120")
    assert int(fx["ctr1"][2]) >= 100
    assert int((fx["hits0"]["t"].view(np.uint32) != fx["hits1"]["t"].view(np.uint32)).sum()) >= 50


def test_update_pair_shares_objects():
    """spheres1500_b is spheres1500 with every object moved (the update test's second frame)."""
    a, b = T.load_fixture("spheres1500"), T.load_fixture("spheres1500_b")
    assert a["geom"].shape == b["geom"].shape
    assert np.array_equal(a["geom"][:, 12:15], b["geom"][:, 12:15])  # scales
    assert np.all(np.any(a["geom"][:, 0:3] != b["geom"][:, 0:3], axis=1))
