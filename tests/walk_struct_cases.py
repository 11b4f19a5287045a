"""The scenes of tests/test_walk_structs.py and tests/test_gpu_walk_structs.py: small INW scenes
(presets and hand-made boxes, fixed seeds) chosen for where a builder can go wrong, each with what is
expected of it, stated here in advance:

  ri_grid  1 the surrounding-RI grid is built, 0 it is dropped (some cell would list more than 64
           objects).  Only the pile of identical boxes is expected to drop it.
  build    rt_debug_wide_info info[7] after a device update: 1 built on the device, 2 on the host after
           the device build ran past its level cap.  The cap is 256 SAH levels and no scene here has
           more than 2000 well-spread objects or a chain longer than 200, so every scene expects 1
           (the fallback is reached with a lowered cap in the GPU file).
"""
from dataclasses import dataclass

import numpy as np

import rt_amd as R


@dataclass
class Case:
    name: str
    geom: np.ndarray            # (n, 28) GeometryBuff records
    aabbs: np.ndarray           # (n, 6)
    layout: int = 1
    lights: np.ndarray | None = None
    ri_grid: int = 1
    build: int = 1
    _nodes: np.ndarray | None = None

    @property
    def n(self):
        return len(self.aabbs)

    @property
    def nodes(self):
        """The host LBVH over the boxes (cached)."""
        if self._nodes is None:
            self._nodes = R.lbvh_build(self.aabbs)
        return self._nodes

    @property
    def moving(self):
        return bool((self.geom[:, 15:18] != 0).any())


def _preset(name, preset, seed, n_hint, **kw):
    sc = R.make_scene(preset, seed, n_hint, width=8, height=8, spp=1)
    return Case(name, np.ascontiguousarray(sc.geom, np.float32), np.ascontiguousarray(sc.aabbs, np.float32),
                layout=sc.layout, lights=sc.lights if sc.n_lights else None, **kw)


def _boxes(name, lo, hi, **kw):
    """Static unrotated ellipsoids filling the boxes [lo, hi] (their AABBs are the boxes)."""
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    n = len(lo)
    g = np.zeros((n, 28), np.float32)
    g[:, 0:3] = (lo + hi) * np.float32(0.5)
    g[:, [3, 7, 11]] = 1.0
    g[:, 12:15] = np.maximum((hi - lo) * np.float32(0.5), np.float32(1e-3))
    g[:, 18] = 1.0   # ellipsoid
    g[:, 20] = 1.5   # refractive index
    g[:, 21:24] = 0.5
    return Case(name, g, np.ascontiguousarray(np.concatenate([lo, hi], axis=1), np.float32), **kw)


def _translated(name, base, offset):
    off = np.asarray(offset, np.float32)
    g, a = base.geom.copy(), base.aabbs.copy()
    g[:, 0:3] += off
    a[:, 0:3] += off
    a[:, 3:6] += off
    return Case(name, g, a, layout=base.layout)


def _make():
    out = []
    out.append(_preset("random600", R.PRESET_INW01_RANDOM, 1234, 600))
    out.append(_preset("random2000", R.PRESET_INW01_RANDOM, 4321, 2000))
    out.append(_preset("grid9", R.PRESET_INW01_GRID, 0, 9))
    out.append(_preset("cornell", R.PRESET_INW04_CORNELL, 7, 0))
    for n in (2, 3, 5, 257, 1025):  # fewer than four children in a node; one past a 256-lane block
        out.append(_preset(f"random{n}", R.PRESET_INW01_RANDOM, 77 + n, n))
    rng = np.random.default_rng(20240611)
    lo = np.tile(np.array([[1.0, 2.0, 3.0]], np.float32), (300, 1))
    out.append(_boxes("dups300", lo, lo + np.float32(1.5), ri_grid=0))  # centroid bins are degenerate
    c = rng.uniform(-40, 40, (400, 3))
    c[:, 2] = 7.0  # coplanar centroids: one axis of the centroid bounds has zero extent
    h = rng.uniform(0.2, 1.0, (400, 1)) * np.ones((1, 3))
    out.append(_boxes("coplanar400", c - h, c + h))
    c = rng.uniform(-30, 30, (500, 3))
    h = rng.uniform(0.1, 0.6, (500, 3))
    out.append(_boxes("spanning501", np.concatenate([[[-32.0, -32.0, -32.0]], c - h]),
                      np.concatenate([[[32.0, 32.0, 32.0]], c + h])))
    x = np.arange(200, dtype=np.float64)[:, None]  # unit boxes along x, each touching the next
    out.append(_boxes("chain200", np.concatenate([x, 0 * x, 0 * x], axis=1), np.concatenate([x + 1, 0 * x + 1, 0 * x + 1], axis=1)))
    base = out[0]
    # coordinates approach +990 in x and -990 in y (the fused cull's condition is 1000)
    off = (990.0 - float(base.aabbs[:, 3].max()), -990.0 - float(base.aabbs[:, 1].min()), 0.0)
    out.append(_translated("random600_at990", base, off))
    # moving rotated unequal-scale ellipsoids and cuboids (tests/cases.py _mixed): the bin boxes come from
    # rotation, scale and delta
    import cases as frames
    for name, sc in (("mixed250", frames.CASES["inw01_mixed_moving"]()), ("mixed120_l4", frames.CASES["inw04_mixed_moving"]())):
        out.append(Case(name, np.ascontiguousarray(sc.geom, np.float32), np.ascontiguousarray(sc.aabbs, np.float32),
                        layout=sc.layout, lights=sc.lights if sc.n_lights else None))
    out.append(_preset("refset5", R.PRESET_INW04_REFSET, 0, 0))  # (not in NAMES: the INW-04 scene updates start from)
    return out


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = _make()
    return _CASES


NAMES = ["random600", "random2000", "grid9", "cornell", "random2", "random3", "random5", "random257", "random1025",
         "dups300", "coplanar400", "spanning501", "chain200", "random600_at990", "mixed250", "mixed120_l4"]


def case(name):
    return next(c for c in cases() if c.name == name)


def qmargin():
    """kQMargin as rt_scene_build.hip defines it (a float literal), as the float64 value of that float."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "raytracing-tests_amd",
                            "csrc", "rt_scene_build.hip")).read()
    m = re.search(r"constexpr\s+float\s+kQMargin\s*=\s*([0-9.eE+-]+)f\s*;", src)
    assert m, "kQMargin not found in rt_scene_build.hip"
    return float(np.float32(float(m.group(1))))


def time_bins(c, bins):
    """rt_debug_time_bins over the case: (n_wtree0, bins built, stride, wnodes (N, 40))."""
    import ctypes as C
    lib = R.load()
    info = (C.c_uint32 * 4)()
    assert lib.rt_debug_time_bins(R.fptr(c.nodes), R.fptr(c.geom), c.n, bins, None, 0, info) == 0
    n0, nb, stride, total = list(info)
    out = np.zeros((total, 40), np.float32)
    assert lib.rt_debug_time_bins(R.fptr(c.nodes), R.fptr(c.geom), c.n, bins, R.fptr(out), total, info) == 0
    return n0, nb, stride, out


def bin_boxes(geom, n, bins, b):
    boxes = np.zeros((n, 6), np.float32)
    assert R.load().rt_debug_bin_boxes(R.fptr(np.ascontiguousarray(geom, np.float32)), n, bins, b, R.fptr(boxes)) == 0
    return boxes
