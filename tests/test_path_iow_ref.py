"""The IOW-03 path-query fixtures (tests/golden/path_iow_*.npz) against their reference, on the CPU:
tests/path_iow_ref.c -- the oracle's own launch_rays() per query on a ray stack that holds the
incoming RI state, cross-checked against a restated loop that tracks stale reads -- is rebuilt and
recomputes every fixture bit for bit; the fixtures reach the ground the GPU tests rely on them for;
the chained answers of a frame's camera rays fold to the oracle's own render; and the `stale` bits
mean what the contract says."""
import numpy as np
import pytest

import path_iow_ref as P
import trace_iow_ref as T


@pytest.fixture(scope="module")
def ref_lib(tmp_path_factory):
    return P.build(tmp_path_factory.mktemp("path_iow_ref"))


def scene_of(fx):
    s = T.load_fixture(str(fx["scene"]))
    return s["types"], s["records"]


@pytest.mark.parametrize("name", P.SETS)
def test_fixture_recomputes_bit_for_bit(ref_lib, name):
    fx = P.load_fixture(name)
    types, rec = scene_of(fx)
    out, ctr = P.run(ref_lib, types, rec, fx["rays"], fx["max_bounces"], fx["chain"])
    assert P.same(out, fx["out"]), name
    assert np.array_equal(ctr, fx["ctr"])
    ran = out["status"] == 0
    assert ctr[0] == out["segments"].sum() and ctr[1] == out["drops"].sum() and ctr[2] == out["nans"].sum()
    assert np.all(out["segments"][ran] >= 1) and not out["segments"][~ran].any()


def test_fixtures_reach_the_new_ground():
    """The floors the generator asserts, on the committed files."""
    f = {name: P.load_fixture(name)["out"] for name in P.SETS}
    assert (f["final"]["stale"] != 0).mean() >= 0.05
    assert (f["rot"]["stale"] != 0).mean() >= 0.05
    assert f["shells"]["nans"].sum() > 0 and (f["shells"]["drops"] > 0).mean() > 0.5
    assert f["final_deep"]["segments"].max() > 1000
    st = P.load_fixture("state")
    assert (st["out"]["status"] == 1).sum() == 24 and np.all(st["rays"]["sample"][st["out"]["status"] == 1] >= P.SPP)
    assert st["chain"] == 1 and st["rays"]["ri_in"].any(1).all()
    d2 = (st["rays"]["d"].astype(np.float64) ** 2).sum(1)
    assert (d2 == 0).sum() >= 10 and np.isnan(d2).sum() >= 10 and ((d2 > 1.002) | (d2 < 0.998)).sum() >= 100
    for name in ("final", "final_deep", "rot", "ref3", "shells", "one", "cam_final"):
        assert P.load_fixture(name)["chain"] == 8
    assert len(f["final"]) == 4800 and len(f["final_deep"]) == 512 and len(f["cam_final"]) == P.CAM_W * P.CAM_H * P.SPP


def test_rot_chained_answers_depend_on_the_state(ref_lib):
    """At least 5% of rot's chained queries differ in rgb from the same ray with the zero state."""
    fx = P.load_fixture("rot")
    types, rec = scene_of(fx)
    zero = fx["rays"].copy()
    zero["ri_in"] = 0.0
    alone, _ = P.run(ref_lib, types, rec, zero, fx["max_bounces"], 1)
    later = np.arange(len(zero)) % fx["chain"] != 0
    differ = (alone["rgb"].view(np.uint32) != fx["out"]["rgb"].view(np.uint32)).any(1)
    assert differ[later].mean() >= 0.05
    # a chain's first query does see its own ri_in, here zero
    assert P.same(alone[~later], fx["out"][~later])
    # ... and a path that read no incoming value answers the same with any state
    clean = later & (fx["out"]["stale"] == 0)
    assert clean.sum() > 1000
    assert np.array_equal(alone["rgb"][clean].view(np.uint32), fx["out"]["rgb"][clean].view(np.uint32))


def test_chain_is_the_host_feeding_the_state_forward(ref_lib):
    fx = P.load_fixture("rot")
    types, rec = scene_of(fx)
    rays = fx["rays"].reshape(-1, 8).copy()
    state = rays["ri_in"][:, 0].copy()
    for j in range(8):
        step = rays[:, j].copy()
        step["ri_in"] = state
        out, _ = P.run(ref_lib, types, rec, step, fx["max_bounces"], 1)
        assert P.same(out, fx["out"].reshape(-1, 8)[:, j].copy()), j
        state = out["ri_out"]


def test_folded_camera_chains_are_the_oracle_frame(ref_lib):
    """cam_final's chained answers fold to orc_render_iow03 of the 16 x 9 frame, with its totals: the
    camera restatement and the chain rule against the oracle's own render."""
    fx = P.load_fixture("cam_final")
    types, rec = scene_of(fx)
    rays = P.camera_rays(ref_lib, fx["camera"], P.CAM_W, P.CAM_H, P.SPP)
    assert P.same(rays, fx["rays"])
    rgb, st = P.oracle_frame(ref_lib, types, rec, fx["camera"], P.CAM_W, P.CAM_H, P.SPP, fx["max_bounces"])
    assert P.same(P.fold(fx["out"], P.SPP), rgb)
    assert (st["segments"], st["stack_drops"], st["nan_drops"]) == tuple(int(x) for x in fx["ctr"])


def test_fold_stops_at_the_early_return_marker():
    """A status = 1 answer at sample s ends its pixel there, scaled by RN(1 / s) (03...glsl:396)."""
    out = np.zeros(8, P.OUT_DTYPE)
    out["rgb"] = np.arange(24, dtype=np.float32).reshape(8, 3)
    out["status"][[3, 6]] = 1
    want = (out["rgb"][0] + out["rgb"][1] + out["rgb"][2]) * (np.float32(1.0) / np.float32(3))
    assert P.same(P.fold(out, 8), want[None, :])


def test_clear_stale_bits_mean_independence(ref_lib):
    """`state` again with other ri_in values in every slot whose stale bit is clear: rgb, the counts and
    stale keep their bits; ri_out changes only where the path left the slot unwritten."""
    fx = P.load_fixture("state")
    types, rec = scene_of(fx)
    rays, want = fx["rays"].copy(), fx["out"]
    clear = ((want["stale"][:, None] >> np.arange(4)) & 1) == 0
    rays["ri_in"][clear] = (rays["ri_in"][clear] + np.float32(0.7)) * np.float32(1.9)
    out, ctr = P.run(ref_lib, types, rec, rays, fx["max_bounces"], 1)
    for k in ("rgb", "stale", "segments", "drops", "nans", "status"):
        assert P.same(out[k], want[k]), k
    changed = out["ri_out"].view(np.uint32) != want["ri_out"].view(np.uint32)
    assert not changed[~clear].any()
    assert np.array_equal(out["ri_out"][changed].view(np.uint32), rays["ri_in"][changed].view(np.uint32))
    assert changed.any() and (want["stale"] != 0).sum() > 100
    # ... while the stale slots matter: zeroing them changes some answer
    rays = fx["rays"].copy()
    rays["ri_in"][~clear] = 0.0
    out, _ = P.run(ref_lib, types, rec, rays, fx["max_bounces"], 1)
    assert (out["rgb"].view(np.uint32) != want["rgb"].view(np.uint32)).any()
