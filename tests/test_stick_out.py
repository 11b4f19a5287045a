"""Objects inside their leaf boxes: the measure that decides per scene whether the wide
walk applies (rtamd::inw_stick_out through rt_debug_inw_stick_out), on the CPU.  Every scene the
packers produce lies far below the margin, so C3, C5 and every test scene keep their path; the shrunk
caller boxes lie far above it; and the measure agrees with the objects' own surface points
(walk_struct_ref.inw_samples, which shares no code with the library)."""
import glob
import os

import numpy as np
import pytest

import rt_amd as R
import walk_struct_cases as K
import walk_struct_ref as W
from cases import CASES, SHRUNK_CASES

INW = sorted(n for n in CASES if n.startswith("inw"))


@pytest.mark.parametrize("name", INW)
def test_frame_cases(name):
    sc = CASES[name]()
    by_nodes, by_boxes = R.inw_stick_out(sc.geom, nodes=sc.nodes), R.inw_stick_out(sc.geom, aabbs=sc.aabbs)
    print(name, by_nodes, by_boxes)
    assert by_nodes == by_boxes  # the LBVH's leaves are the boxes
    if name in SHRUNK_CASES:
        assert by_nodes > 100.0
    else:
        # the packers round their boxes to float32: an object sticks out by an ulp or so of its
        # coordinates (6e-8 relative) against the margin's 1e-5
        assert by_nodes < 0.05


def test_structure_cases_and_fixtures():
    for c in K.cases():
        assert R.inw_stick_out(c.geom, nodes=c.nodes) < 0.05, c.name
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    seen = 0
    for path in sorted(glob.glob(os.path.join(golden, "*.npz"))):
        with np.load(path) as z:
            if not {"geom", "nodes"} <= set(z.files) or z["geom"].ndim != 2 or z["geom"].shape[1] != 28:
                continue
            v = R.inw_stick_out(z["geom"], nodes=z["nodes"])
        seen += 1
        if "shrunk" in os.path.basename(path):
            assert v > 100.0, path
        else:
            assert v < 0.05, path
    assert seen >= 20


def test_bench_scenes():
    """The C3 and C5 scenes of bench.py (the presets at their full object counts)."""
    for preset, seed, n in ((R.PRESET_INW01_RANDOM, 1234, 10000), (R.PRESET_INW04_CORNELL, 7, 0)):
        sc = R.make_scene(preset, seed, n, width=8, height=8, spp=1)
        assert R.inw_stick_out(sc.geom, nodes=sc.nodes) < 0.05


def test_measure_follows_the_geometry():
    """Against surface samples: boxes made of each object's own samples over the shutter interval
    (both end ratios) hold the object up to rounding; one face moved inward by k margins measures k."""
    c = K.case("mixed250")
    own = W.inw_sample_boxes(c.geom, (0.0, 1.0), W.unit_dirs(50))
    lo, hi = own[:, 0:3].astype(np.float32), own[:, 3:6].astype(np.float32)
    lo = np.where(lo > own[:, 0:3], np.nextafter(lo, np.float32(-np.inf)), lo)  # rounded outward
    hi = np.where(hi < own[:, 3:6], np.nextafter(hi, np.float32(np.inf)), hi)
    boxes = np.ascontiguousarray(np.concatenate([lo, hi], axis=1), np.float32)
    assert R.inw_stick_out(c.geom, aabbs=boxes) < 1e-6  # (float32 record arithmetic against float64 samples)
    for g, col, k in ((10, 0, 3.0), (11, 4, 0.5), (200, 5, 40.0), (201, 2, 1.5)):  # ellipsoids and cuboids
        b = boxes.copy()
        margin = 1e-5 * max(1.0, float(np.abs(b[g]).max()))
        b[g, col] = np.float32(float(b[g, col]) + k * margin * (1 if col < 3 else -1))
        got = R.inw_stick_out(c.geom, aabbs=b)
        assert abs(got - k) < 0.02, (g, col, k, got)
        assert (got <= 1.0) == (k <= 1.0)


def test_measure_reads_the_leaves_of_a_node_buffer():
    c = K.case("mixed250")
    nodes = c.nodes.copy()
    leaf = W.lbvh_leaves(nodes, c.n)
    assert R.inw_stick_out(c.geom, nodes=nodes) < 0.05
    own = W.inw_sample_boxes(c.geom[17:18], (0.0, 1.0), W.unit_dirs(50))[0]
    nodes[leaf[17], 3] = np.float32(own[3] - 0.25)  # object 17's leaf: the +x face a quarter unit inside the object
    v = R.inw_stick_out(c.geom, nodes=nodes)
    want = (own[3] - float(nodes[leaf[17], 3])) / (1e-5 * max(1.0, float(np.abs(nodes[leaf[17], 0:6]).max())))
    assert abs(v - want) < 1e-3 * want and v > 1000.0
    inner = np.flatnonzero(nodes[:, 6] > 0.1)[3]
    nodes = c.nodes.copy()
    nodes[inner, 0:6] = 0.0  # an inner node's box is not an object's
    assert R.inw_stick_out(c.geom, nodes=nodes) < 0.05


def test_values_that_are_not_finite():
    c = K.case("random5")
    for col in (0, 12, 15):
        g = c.geom.copy()
        g[2, col] = np.nan
        assert R.inw_stick_out(g, nodes=c.nodes) == np.inf
    b = c.aabbs.copy()
    b[1, 4] = np.inf  # a box that holds everything along y: nothing sticks out of it
    assert R.inw_stick_out(c.geom, aabbs=b) < 0.05
    lib = R.load()
    assert lib.rt_debug_inw_stick_out(None, 5, None, None, None) == R.RT_E_ARG
