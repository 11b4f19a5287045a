"""The wide walk's leaf takes (csrc/rt_inw_walk.hpp: inw_traverse_wide takes a node step's
nearest-child leaf in the step's own trip) on the GPU: rt_trace_inw's answers (t, object, normal,
record float 19) bit for bit against the same queries on a scene built with inw_wide_walk = 0 (the
reference's walk), for both child orders, inw_qnodes 0 and 1 and inw_time_bins 0 and 2.  What the
scenes hold (a root with only leaves, a nearest leaf beside farther nodes and the reverse, leaves
stacked on each other, a popped leaf that has to wait, the stack running empty in a taking trip,
lanes that take in the first trip beside lanes that walk on, an overflow in a taking trip) is
asserted on the CPU by tests/test_walk_takes_ref.py.  One small C3 frame against the oracle."""
import numpy as np
import pytest

import rt_amd as R
import walk_takes_cases as K
from oracle import oracle as O
from test_gpu_trace import assert_same

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

_scenes, _refs = {}, {}


def _scene(key):
    if key not in _scenes:
        _scenes[key] = K.chain_scene() if key == "chain" else K.small_scene(key)
    return _scenes[key]


def _reference(key, invert):
    """The reference walk's answers on the GPU (inw_wide_walk = 0), computed once per scene and order."""
    if (key, invert) not in _refs:
        sc = _scene(key)
        with R.options(inw_wide_walk=0):
            hits, st = R.trace(sc, sc.rays, invert * R.RT_TRACE_INVERT)
        assert st["segments"] == len(sc.rays) and st["stack_drops"] == 0
        hits.setflags(write=False)
        _refs[(key, invert)] = hits
    return _refs[(key, invert)]


@pytest.mark.parametrize("time_bins", [0, 2])
@pytest.mark.parametrize("qnodes", [0, 1])
@pytest.mark.parametrize("invert", [0, 1])
@pytest.mark.parametrize("key", list(K.SIZES) + ["chain"])
def test_takes_match_the_reference_walk(gpu, key, invert, qnodes, time_bins):
    sc = _scene(key)
    want = _reference(key, invert)
    with R.options(inw_qnodes=qnodes, inw_time_bins=time_bins):
        hits, st = R.trace(sc, sc.rays, invert * R.RT_TRACE_INVERT)
    assert_same(hits, want, f"{key} objects, invert {invert}, qnodes {qnodes}, time bins {time_bins}")
    assert st["segments"] == len(sc.rays) and st["stack_drops"] == 0 and st["nan_drops"] == 0
    if key != "chain":
        assert (hits["id"] >= 0).sum() >= 32


@pytest.mark.parametrize("invert", [0, 1])
def test_mixed_waves_in_windows(gpu, invert):
    """Windows of the 5-object queries that start inside a wave: other lanes beside the ones that
    take a leaf in the first trip, and partial waves."""
    sc = _scene(5)
    want = _reference(5, invert)
    for lo, k in ((0, 1), (0, 63), (0, 65), (7, 64), (130, 126)):
        hits, st = R.trace(sc, sc.rays[lo:lo + k], invert * R.RT_TRACE_INVERT)
        assert_same(hits, want[lo:lo + k], f"[{lo}:{lo + k}] invert {invert}")
        assert st["segments"] == k


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def test_small_c3_frame_matches_the_oracle(gpu):
    """The C3 preset with 200 objects, 64 x 36 at 8 spp: colour, depth and the exact counters."""
    sc = R.make_scene(R.PRESET_INW01_RANDOM, 1234, 200, width=64, height=36, spp=8)
    rgba, depth, st = R.render(sc, sc.params)
    orgba, odepth, ost = O.render(sc, sc.params)
    assert _same(rgba, orgba), "colour differs from the oracle"
    assert _same(depth, odepth), "depth differs from the oracle"
    for k in ("segments", "stack_drops", "nan_drops"):
        assert st[k] == ost[k], (k, st[k], ost[k])
    assert st["segments"] > 64 * 36 * 8
