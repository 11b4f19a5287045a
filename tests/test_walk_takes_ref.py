"""The cases tests/test_gpu_walk_takes.py relies on, asserted on the CPU with a model of one lane of
the wide walk (walk_takes_cases.lane_events over the host-built 4-wide nodes), and the CPU
reference (tests/trace_ref.c) on the same queries: the scenes are answered with hits and misses."""
import collections

import numpy as np
import pytest

import trace_ref as T
import walk_takes_cases as K


@pytest.fixture(scope="module")
def ref_lib(tmp_path_factory):
    return T.build(tmp_path_factory.mktemp("trace_ref"))


def _count(ev):
    return collections.Counter(e for s, _ in ev for e in s)


def test_root_is_a_leaf_or_holds_only_leaves():
    sc = K.small_scene(1)
    assert sc.nodes.shape == (1, 8) and not sc.nodes[0, 6] > 0.1  # the LBVH root is a leaf
    for n in (2, 3):
        ev, links, info = K.events_of(K.small_scene(n))
        assert info["wide_nodes"] == 1 and int(np.sum(links[0] <= 0)) == n  # the root's children are all leaves
        c = _count(ev)
        # a lane takes a leaf in the root's own trip or misses every child; the stack runs empty in a
        # taking trip, and a pop brings up the second leaf while the lane holds the first
        assert c["step_take"] + c["empty_after_miss"] == len(ev) and c["empty_after_miss"] >= 16
        assert c["empty_in_taking_trip"] >= 64 and c["popped_leaf_waits"] >= 16


@pytest.mark.parametrize("n", [5, 17])
def test_mixed_children_and_stacked_leaves(n):
    ev, links, info = K.events_of(K.small_scene(n))
    assert info["wide_nodes"] >= 2 and 0 < info["dfs_high"] <= 40
    c = _count(ev)
    for k in ("near_leaf_far_node", "near_node_far_leaf", "leaf_under_leaf", "popped_leaf_waits", "near_leaf_waits",
              "empty_in_taking_trip", "popped_leaf_free"):
        assert c[k] >= 2, (k, dict(c))
    if n == 5:
        assert c["free_leaf_over_leaf"] + c["popped_leaf_last"] >= 2, dict(c)
        # in every wave some lanes take a leaf in the first trip while others step on to a node
        for w in range(0, len(ev), 64):
            first = collections.Counter(t[0] for _, t in ev[w:w + 64])
            assert first["take"] >= 16 and first["step"] >= 16, (w, dict(first))


def test_overflow_in_a_taking_trip():
    sc = K.chain_scene()
    ev, _, info = K.events_of(sc)
    assert 0 < info["dfs_high"] <= 40  # the walk's own condition holds: the overflow is the walk stack's
    for w in range(0, len(ev), 64):
        c = _count(ev[w:w + 64])
        assert c["overflow_taking"] >= 8, (w, dict(c))
        over = sum(1 for s, _ in ev[w:w + 64] if "overflow_taking" in s or "overflow_other" in s)
        assert over <= 48  # beside lanes that do not overflow


@pytest.mark.parametrize("n", K.SIZES)
def test_reference_answers_hits_and_misses(ref_lib, n):
    sc = K.small_scene(n)
    for invert in (0, 1):
        hits, ctr = T.run(ref_lib, sc.geom, sc.nodes, sc.layout, sc.rays, invert)
        assert int(ctr[2]) == 0
        hit = hits["id"] >= 0
        assert hit.sum() >= 32 and (n > 5 or (~hit).sum() >= 8), (n, int(hit.sum()))
