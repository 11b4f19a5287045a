"""The progressive passes' reference (tests/pass_ref.py) on the CPU: the prefix fold at k = spp is the
oracle's frame of the fixture's scene, so the reference is tied to oracle/; and a fold cut at any k and
continued from the state gives the bytes of the uncut fold."""
import numpy as np
import pytest

import pass_ref as PR
import path_iow_ref as PI
import path_ref as P
import rt_amd as R
import trace_iow_ref as T
from oracle import oracle as O

NAMES = PR.INW + [PR.IOW]


def preset_scene(name):
    """The preset scene the fixture was generated from, with the fixture's bounce limit."""
    if name == PR.IOW:
        fx = PI.load_fixture(name)
        sc = R.make_scene(R.PRESET_IOW03_FINAL, 20250131, 0, width=PR.W, height=PR.H, spp=PI.SPP)
        assert np.array_equal(sc.records, T.load_fixture(str(fx["scene"]))["records"])
        assert bytes(sc.camera) == fx["camera"].tobytes() and sc.params.max_bounces == fx["max_bounces"]
        return sc
    fx = P.load_fixture(name)
    if name == "cam_random600":
        sc = R.make_scene(R.PRESET_INW01_RANDOM, 1234, 600, width=PR.W, height=PR.H, spp=P.SPP)
    else:
        sc = R.make_scene(R.PRESET_INW04_CORNELL, width=PR.W, height=PR.H, spp=P.SPP)
    assert np.array_equal(sc.geom, fx.geom) and bytes(sc.camera) == fx.camera.tobytes()
    sc.params.max_bounces = fx.max_bounces
    return sc


@pytest.mark.parametrize("name", NAMES)
def test_full_fold_is_the_oracle_frame(name):
    spp = PR.spp_of(name)
    rgba, depth = PR.image(PR.state(name, spp), spp)
    want, wdepth, st = O.render(preset_scene(name))
    assert P.same(rgba, want.reshape(-1, 4).copy())
    if name != PR.IOW:
        assert P.same(depth, wdepth.reshape(-1).copy())
    else:
        assert not depth.any()
    c = PR.counters(name, 0, spp)
    assert c[0] == st["segments"] and c[4] == st["stack_drops"] and c[5] == st["nan_drops"]


@pytest.mark.parametrize("name", NAMES)
def test_a_fold_cut_anywhere_continues_to_the_same_bytes(name):
    spp = PR.spp_of(name)
    out = PR.samples(name)
    whole = [PR.state(name, k) for k in range(spp + 1)]
    for k in range(1, spp):
        head = PR.fold(name, out, 0, k)
        assert P.same(head, whole[k]), k
        for k1 in (k + 1, spp):
            assert P.same(PR.fold(name, out, k, k1, head), whole[k1]), (k, k1)
    # three ranges, and a state buffer that held other bytes before the first range
    junk = np.frombuffer(bytes([0xCD]) * (len(out) * 32), PR.STATE_DTYPE)
    a = PR.fold(name, out, 0, 3, junk)
    assert P.same(PR.fold(name, out, spp // 2, spp, PR.fold(name, out, 3, spp // 2, a)), whole[spp])


@pytest.mark.parametrize("name", NAMES)
def test_states_are_what_the_contract_says(name):
    spp = PR.spp_of(name)
    out = PR.samples(name)
    for k in range(1, spp + 1):
        st = PR.state(name, k)
        if name == PR.IOW:
            assert not st["depth"].any()
            assert P.same(st["ri"], np.ascontiguousarray(out["ri_out"][:, k - 1]))
        else:
            assert not st["ri"].any()
            if k <= spp // 2:
                assert not st["depth"].any()  # sample spp / 2 has not run
            else:
                assert P.same(st["depth"], np.ascontiguousarray(out["depth"][:, spp // 2]))
    if name != PR.IOW:
        assert PR.state(name, spp)["depth"].any()  # the frames see the sky: a depth of 0 would prove nothing
    else:
        assert len(np.unique(PR.state(name, spp)["ri"])) > 2  # the pixels leave different RI states behind
