"""The ray-query fixtures (tests/golden/trace_*.npz) against their reference, on the CPU:
tests/trace_ref.c -- the oracle's own closest-hit walk per query -- is rebuilt and recomputes
every fixture bit for bit, and the fixtures exercise what the GPU tests rely on them for: hits
and misses in every scene, exact ties decided by the child order (dups300), pushes the full
40-float stack drops (pile120), and caller boxes that the objects stick out of, where the winner depends
on the child order and lies far in front of its own leaf box (shrunk06, shrunk09)."""
import numpy as np
import pytest

import trace_ref as T


SHRUNK = ("shrunk06", "shrunk09")  # objects stick out of their boxes (test_shrunk_boxes_are_adversarial)


@pytest.fixture(scope="module")
def ref_lib(tmp_path_factory):
    return T.build(tmp_path_factory.mktemp("trace_ref"))


@pytest.mark.parametrize("name", T.SCENES)
def test_fixture_recomputes_bit_for_bit(ref_lib, name):
    fx = T.load_fixture(name)
    n = fx["geom"].shape[0]
    assert fx["geom"].shape == (n, 28) and fx["nodes"].shape == (2 * n - 1, 8) and fx["aabbs"].shape == (n, 6)
    assert fx["rays"].shape == (4096 if name in SHRUNK else 2048,) and fx["layout"] in (1, 4)
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
    # the child order changes no hit mask unless a push dropped (objects inside their boxes)
    if not fx["ctr0"][2] and not fx["ctr1"][2] and name not in SHRUNK:
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


def _winner_box_entry(fx, hits):
    """(entry t of each winner's own leaf box along its ray, the winner's t), float64, for the hits."""
    rays, hit = fx["rays"], hits["id"] >= 0
    box = fx["aabbs"][hits["id"][hit]].astype(np.float64)
    o, d = rays["o"][hit].astype(np.float64), rays["d"][hit].astype(np.float64)
    with np.errstate(all="ignore"):
        near = np.minimum((box[:, 0:3] - o) / d, (box[:, 3:6] - o) / d)
    return np.where(d != 0, near, -np.inf).max(axis=1), hits["t"][hit].astype(np.float64)


def test_shrunk_boxes_are_adversarial():
    """What the shrunk-box fixtures are for.  The reference tests a leaf box against its running limit,
    so with boxes the objects stick out of its answer depends on the child order; and a winner can lie
    far in front of its own leaf box: beyond the wide walk's culling limit t * 1.0001 + 1e-3, which the
    leaf-entry guard's argument assumes never happens.  With the packers' own boxes
    (mixed700) neither occurs."""
    fx = T.load_fixture("shrunk06")
    assert fx["geom"].shape[0] == 200 and int((fx["geom"][:, 15:18] != 0).any(axis=1).sum()) > 100
    assert int((fx["hits0"]["id"] != fx["hits1"]["id"]).sum()) >= 100
    for name, least in (("shrunk06", 500), ("shrunk09", 100)):
        fx = T.load_fixture(name)
        for k in ("hits0", "hits1"):
            te, t = _winner_box_entry(fx, fx[k])
            assert int((te > t * 1.0001 + 1e-3).sum()) >= least, (name, k)
    fx = T.load_fixture("mixed700")
    assert np.array_equal(fx["hits0"]["id"], fx["hits1"]["id"])
    for k in ("hits0", "hits1"):
        te, t = _winner_box_entry(fx, fx[k])
        assert int((te > t * 1.0001 + 1e-3).sum()) == 0
