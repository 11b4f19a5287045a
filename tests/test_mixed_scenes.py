"""What makes the mixed moving cases of tests/cases.py worth rendering, from the oracle alone (no GPU):
objects are hit and missed, rays bounce, lights are sampled, the objects are the moving, rotated,
unequal-scale kind with cuboids among them (so no sphere records), their motion shows in the frame, and
the shrunk caller boxes change what the reference computes."""
import numpy as np
import pytest

import rt_amd as R
from cases import CASES, MIXED_CASES, SHRUNK_CASES, _mixed01, _mixed04
from oracle import oracle as O

_frames = {}


def _oracle(name, make=None):
    if name not in _frames:
        sc = (make or CASES[name])()
        _frames[name] = (sc,) + tuple(O.render(sc))
    return _frames[name]


def _hit(depth):
    return depth < depth.max()  # misses carry the far distance


def _differs(a, b):
    return ((a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))).any(axis=-1)


@pytest.mark.parametrize("name", MIXED_CASES)
def test_mixed_case_is_worth_rendering(name):
    sc, rgba, depth, st = _oracle(name)
    p = sc.params
    assert depth.max() == np.float32(32000.0)
    hit = _hit(depth)
    print(name, "hit fraction", hit.mean(), {k: st[k] for k in ("segments", "shadow_queries", "stack_drops", "nan_drops")})
    assert hit.mean() >= 0.15
    primaries = p.width * p.height * p.spp
    if sc.stage == R.RT_STAGE_INW01:
        # INW-01 splits a ray at a surface (reflection and refraction both go on the ray stack)
        assert st["segments"] >= 1.5 * primaries
        assert st["shadow_queries"] == 0
    else:
        # INW-04 follows one ray per bounce and ends at a light, so with the 28% to 43% of hit pixels
        # these 120 objects give its segments stay below 1.5 primaries (1.15 to 1.42 over seeds 1..16,
        # whatever the material strengths); what its frame is for is the shadow queries with a time
        # ratio, beside moving lights
        assert st["segments"] > primaries and st["shadow_queries"] > 0
        assert sc.n_lights >= 2
        lights = np.flatnonzero([sc.desc[i].emissive for i in range(sc.n)])
        assert any(tuple(sc.desc[i].position) != tuple(sc.desc[i].last_position) for i in lights)
    if (p.width, p.height) == (96, 64):  # the full INW-01 frames (the 33x21 frame has 15 blocks in all)
        blocks = hit.reshape(8, 8, 12, 8).any(axis=(1, 3))
        assert blocks.sum() >= 10 and (~blocks).sum() >= 10  # beam lists to build, and sky blocks
    g = sc.geom
    general = ((g[:, 15:18] != 0).any(axis=1) & (g[:, [4, 5, 6, 8, 9, 10]] != 0).any(axis=1) &
               ((g[:, 12] != g[:, 13]) | (g[:, 13] != g[:, 14])))
    assert general.sum() > sc.n / 3
    assert ((g[general, 18] + 0.1).astype(int) == R.RT_INW_CUBOID).sum() > sc.n / 10
    out = np.zeros((sc.n, 12), np.float32)
    assert R.load().rt_debug_sphere_records(R.fptr(np.ascontiguousarray(g)), sc.n, sc.layout, R.fptr(out)) == 0


def test_back_view_takes_the_other_child_order():
    """The reference walk orders children by the sign of dot(camera direction, 1)."""
    front, back = CASES["inw01_mixed_moving"](), CASES["inw01_mixed_moving_back"]()
    assert sum(front.camera.dir) > 0 > sum(back.camera.dir)
    assert front.geom.tobytes() == back.geom.tobytes() and front.nodes.tobytes() == back.nodes.tobytes()


@pytest.mark.parametrize("name,make", [("inw01_mixed_moving", _mixed01), ("inw04_mixed_moving", _mixed04)])
def test_motion_matters(name, make):
    """The same objects with every last_position = position: at least 5% of the hit pixels differ."""
    sc, rgba, depth, _ = _oracle(name)
    still, rgba0, _, _ = _oracle(name + ":static", lambda: make(static=True))
    assert not (still.geom[:, 15:18] != 0).any() and np.array_equal(still.geom[:, 0:15], sc.geom[:, 0:15])
    hit = _hit(depth)
    frac = (_differs(rgba, rgba0) & hit).sum() / hit.sum()
    print(name, "hit pixels that differ without motion", frac)
    assert frac >= 0.05


@pytest.mark.parametrize("name", SHRUNK_CASES)
def test_shrunk_boxes_decide(name):
    """The reference culls with the boxes it is given: with boxes the objects stick out of, its frame
    differs from the frame with the packers' boxes (the same geometry record for record) in more than
    1% of the pixels."""
    full = {"inw01_mixed_shrunk06": "inw01_mixed_moving", "inw01_mixed_shrunk06_back": "inw01_mixed_moving_back",
            "inw04_mixed_shrunk09": "inw04_mixed_moving"}[name]
    sc, rgba, _, _ = _oracle(name)
    ref, rgba0, _, _ = _oracle(full)
    assert sc.geom.tobytes() == ref.geom.tobytes() and sc.aabbs.tobytes() != ref.aabbs.tobytes()
    n = int(_differs(rgba, rgba0).sum())
    print(name, "pixels that differ from the full-box frame", n)
    assert n > 0.01 * rgba.shape[0] * rgba.shape[1]
