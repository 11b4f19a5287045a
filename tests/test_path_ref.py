"""The path-query fixtures (tests/golden/paths_*.npz) against their reference, on the CPU:
tests/path_ref.c -- the oracle's sample loop restarted from a given ray -- is rebuilt and recomputes
every fixture bit for bit; fed the camera rays it forms itself it equals the oracle's inw_sample,
sample by sample; and folding those samples as End() does reproduces the oracle's frames.  The
fixtures exercise what the GPU tests rely on them for: dropped pushes, NaN directions, shadow rays
and paths of a few hundred segments next to paths of one."""
import numpy as np
import pytest

import path_ref as P
import rt_amd as R
from oracle import oracle as O


@pytest.fixture(scope="module")
def ref_lib(tmp_path_factory):
    return P.build(tmp_path_factory.mktemp("path_ref"))


@pytest.mark.parametrize("name", P.SCENES)
def test_fixture_recomputes_bit_for_bit(ref_lib, name):
    fx = P.load_fixture(name)
    n = fx.n
    assert fx.geom.shape == (n, 28) and fx.nodes.shape == (2 * n - 1, 8) and fx.aabbs.shape == (n, 6)
    assert fx.spp == P.SPP and fx.layout in (1, 4)
    assert len(fx.rays) == (P.CAM_W * P.CAM_H * P.SPP if name in P.CAM else 2048)
    assert np.array_equal(fx.rays["sample"], np.arange(len(fx.rays)) % P.SPP)
    for inv in (0, 1):
        out, ctr = P.run(ref_lib, fx, fx.rays, inv)
        assert P.same(out, fx.out[inv]), (name, inv)
        assert np.array_equal(ctr, fx.ctr[inv]), (name, inv)


@pytest.mark.parametrize("name", P.SCENES)
def test_fixture_outputs_are_well_formed(name):
    fx = P.load_fixture(name)
    for inv in (0, 1):
        o, ctr = fx.out[inv], fx.ctr[inv]
        assert np.isfinite(o["rgb"]).all() and not o["status"].any()
        assert np.all(o["segments"] >= 1) and int(o["segments"].sum()) == int(ctr[0]) <= 1_000_000
        assert int(o["drops"].sum()) == int(ctr[4]) and int(o["nans"].sum()) == int(ctr[5])
        # depth is written by a miss only: 0, or the primary limit when the query itself missed
        one = o["segments"] == 1
        assert np.all(np.isin(o["depth"][one], (0.0, 32000.0)))
        if fx.layout == 1:
            assert ctr[3] == 0


def test_fixtures_cover_the_hard_cases():
    fxs = {name: P.load_fixture(name) for name in P.SCENES}
    pile = fxs["pile100"]
    assert pile.ctr[0][4] == 0 and pile.ctr[1][4] > 100_000         # drops under one child order only
    assert int((pile.out[1]["drops"] > 0).sum()) > 1000
    assert not P.same(pile.out[0], pile.out[1])
    for inv in (0, 1):
        seg = pile.out[inv]["segments"]
        assert seg.max() >= 100 and seg.min() == 1                  # long paths next to 1-segment paths
    assert fxs["glass600"].ctr[0][5] > 0 and fxs["mixed300"].ctr[0][5] > 0   # NaN directions
    assert fxs["cornell"].ctr[0][3] > 0 and fxs["refset_tex"].ctr[0][3] > 0  # shadow rays
    for name in ("cornell", "refset_tex"):                          # half camera rays: paths go on
        assert (fxs[name].out[0]["segments"] > 1).mean() > 0.25
    tex = fxs["refset_tex"]
    assert len(tex.textures) == 2 and sorted(tex.geom[:, 27].tolist())[-2:] == [1.0, 2.0]
    assert np.any(fxs["glass600"].rays["pad"] != 0)                 # pad is ignored: arbitrary bits


def test_update_pair_shares_objects():
    a, b = P.load_fixture("glass600"), P.load_fixture("glass600_b")
    assert a.geom.shape == b.geom.shape
    assert np.array_equal(a.geom[:, 12:15], b.geom[:, 12:15]) and np.array_equal(a.geom[:, 20:], b.geom[:, 20:])
    assert np.all(np.any(a.geom[:, 0:3] != b.geom[:, 0:3], axis=1))


def test_invalid_sample_in_the_reference(ref_lib):
    fx = P.load_fixture("one")
    rays = fx.rays[:32].copy()
    rays["sample"][5], rays["sample"][9] = 16, 0xFFFFFFFF
    out, ctr = P.run(ref_lib, fx, rays, 0)
    bad = np.zeros(32, bool)
    bad[[5, 9]] = True
    assert np.all(out["status"][bad] == 1) and not out["status"][~bad].any()
    assert not out[bad].view(np.uint32).reshape(-1, 8)[:, :7].any()
    assert P.same(out[~bad], fx.out[0][:32][~bad]) and ctr[0] == out["segments"].sum()


def _preset_scene(name):
    if name == "cam_random600":
        return R.make_scene(R.PRESET_INW01_RANDOM, 1234, 600, width=P.CAM_W, height=P.CAM_H, spp=P.SPP)
    return R.make_scene(R.PRESET_INW04_CORNELL, width=P.CAM_W, height=P.CAM_H, spp=P.SPP)


@pytest.mark.parametrize("name", P.CAM)
def test_camera_rays_reproduce_inw_sample_and_the_frame(ref_lib, name):
    """The restated loop fed the camera function's rays equals inw_sample on colour, depth and all six
    counters, and the End() fold of those samples is orc_render_inw_tex's image and depth."""
    fx = P.load_fixture(name)
    rays = P.camera_rays(ref_lib, fx.camera, P.CAM_W, P.CAM_H, P.SPP)
    assert P.same(rays, fx.rays)
    inv = P.camera_invert(fx.camera)
    want, wctr = P.inw_samples(ref_lib, fx, fx.camera, P.CAM_W, P.CAM_H)
    assert P.same(fx.out[inv], want)
    assert np.array_equal(fx.ctr[inv], wctr)
    # the frame
    sc = _preset_scene(name)
    assert np.array_equal(sc.geom, fx.geom) and np.array_equal(sc.nodes, fx.nodes)
    sc.params.max_bounces = fx.max_bounces
    rgba, depth, st = O.render(sc)
    rgb, dep = P.fold(fx.out[inv], P.SPP)
    assert P.same(rgb, rgba[..., :3].reshape(-1, 3).copy())
    assert P.same(dep, depth.reshape(-1).copy())
    assert st["segments"] == wctr[0] and st["shadow_queries"] == wctr[3]
    assert st["node_visits"] == wctr[1] and st["prim_tests"] == wctr[2]
