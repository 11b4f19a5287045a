"""The edge-case query fixtures (tests/golden/trace_edges_*.npz, paths_edges_*.npz): their names, the
classes of degenerate rays they hold, loaders, and the comparison rule of the GPU tests.  Written by
tests/golden/make_edge_golden.py from the CPU oracle (tests/trace_ref.py, tests/path_ref.py),
recomputed by tests/test_edge_ref.py, compared with the GPU by tests/test_gpu_query_edges.py."""
import os
from types import SimpleNamespace

import numpy as np

import path_ref as P
import trace_ref as T

GOLDEN = T.GOLDEN
TRACE_SCENES = ["spheres", "mixed", "far"]     # trace_edges_<scene>.npz
PATH_SCENES = ["spheres", "mixed", "far", "refset4"]  # paths_edges_<scene>.npz
BINS = (2, 3, 7, 16)                           # the time-bin counts whose edges b / B the ratio classes sit on
MAX_BOUNCES = 8

# Direction and origin classes (trace and path fixtures).  aimed: the rays are aimed through or beside
# objects with arithmetic that stays finite, so the class must hold both hits and misses (the CPU
# test's 25% / 5% rule).  The others cannot be aimed that way: a NaN, an infinity or an overflow decides
# their answers (1e30 and 3e38: dot(d, d) overflows, so no ellipsoid is hit; 1e30 origins: o + d * t
# rounds the scene away), a zero direction goes nowhere, or the construction fixes the answer (a ray
# from an object's centre always hits it).
CLASSES = {
    "dir_octant": True,      # the 8 sign patterns without a zero
    "dir_pzero": True,       # the 18 sign patterns with one or two components +0.0
    "dir_nzero": True,       # the same with -0.0
    "dir_sub149": True,      # one component 2^-149 (its reciprocal is infinite)
    "dir_sub127": True,      # one component 2^-127 (subnormal, reciprocal 2^127)
    "dir_min126": True,      # one component 2^-126 (the smallest normal float)
    "dir_1e-30": True,
    "dir_1e30": False,
    "dir_3e38": False,
    "dir_nan": False,
    "dir_inf": False,
    "dir_zero": False,       # all three components +-0.0
    "org_plane": True,       # on a leaf-box plane, the direction zero on that axis: the slab value is 0 * inf
    "org_centre": False,     # exactly an object's centre
    "org_900_tiny": True,    # |o| in (900, 1000] on the axis of a 1e-30 / 2^-126 / 2^-127 direction component
    "org_far": True,         # 3000 to 20000 from the target: inside a path's limit of 32000, and far enough
                             # for the object test's t to fall below the hit's own leaf-box entry
    "org_1e6": True,
    "org_1e30": False,
    "org_nan": False,
    "org_inf": False,
    "org_subnormal": True,   # one origin component subnormal
}
# Trace fixtures only: limits and time ratios.
TRACE_CLASSES = {
    "tmax_inf": True,
    "tmax_fltmax": True,
    "tmax_sub149": False,    # no t lies in (0, 2^-149)
    "tmax_min126": False,
    "tmax_hit_below": False,  # one ulp under a known hit's t: that object is out
    "tmax_hit_exact": False,  # t < tmax fails for it too
    "tmax_hit_above": False,  # one ulp over it: that hit stands
    "ratio_edge_B2": True, "ratio_edge_B3": True, "ratio_edge_B7": True, "ratio_edge_B16": True,
    "ratio_below1": True,    # nextafter(1, 0)
    "ratio_negzero": True,   # -0.0
}
PATH_ONLY = {"bad_sample": False}  # sample >= spp: status 1
# the out-of-range time ratios of the rays_ratio / hits_ratio keys
ONE_UP = np.nextafter(np.float32(1.0), np.float32(2.0))
RATIOS_OUT = np.array([-1e-3, -0.5, -1.0, -7.0, ONE_UP, 1.5, 2.0, 9.0, np.inf, -np.inf, np.nan], np.float32)


def trace_class_names():
    return list(CLASSES) + list(TRACE_CLASSES)


def path_class_names():
    return list(CLASSES) + list(PATH_ONLY)


def bin_edge_ratios(B):
    """float(b / B) for b in 1..B-1 with its two neighbours."""
    out = []
    for b in range(1, B):
        r = np.float32(b) / np.float32(B)
        out += [np.nextafter(r, np.float32(-1.0)), r, np.nextafter(r, np.float32(2.0))]
    return np.array(out, np.float32)


def load_trace(name):
    """trace_edges_<name>.npz as a packed scene (what rt_amd.trace takes) with rays, cls (indices into
    names), hits / drops per child order and the same for the out-of-range ratio queries."""
    with np.load(os.path.join(GOLDEN, f"trace_edges_{name}.npz")) as z:
        d = {k: z[k] for k in z.files}
    fx = SimpleNamespace(name=name, geom=d["geom"], aabbs=d["aabbs"], nodes=d["nodes"], layout=int(d["layout"]),
                         rays=d["rays"].view(T.RAY_DTYPE).reshape(-1), cls=d["cls"], names=[str(s) for s in d["names"]],
                         hits=tuple(d[f"hits{i}"].view(T.HIT_DTYPE).reshape(-1) for i in (0, 1)),
                         ctr=(d["ctr0"], d["ctr1"]),
                         rays_ratio=d["rays_ratio"].view(T.RAY_DTYPE).reshape(-1),
                         hits_ratio=tuple(d[f"hits_ratio{i}"].view(T.HIT_DTYPE).reshape(-1) for i in (0, 1)),
                         ctr_ratio=(d["ctr_ratio0"], d["ctr_ratio1"]))
    fx.n = fx.geom.shape[0]
    return fx


def load_paths(name):
    """paths_edges_<name>.npz as path_ref.load_fixture gives the paths_*.npz ones, with cls and names."""
    with np.load(os.path.join(GOLDEN, f"paths_edges_{name}.npz")) as z:
        d = {k: z[k] for k in z.files}
    fx = SimpleNamespace(name=name, geom=d["geom"], aabbs=d["aabbs"], nodes=d["nodes"], layout=int(d["layout"]),
                         lights=d["lights"], n_lights=len(d["lights"]), spp=int(d["spp"]), textures=None,
                         max_bounces=int(d["max_bounces"]), rays=d["rays"].view(P.RAY_DTYPE).reshape(-1),
                         cls=d["cls"], names=[str(s) for s in d["names"]],
                         out=tuple(d[f"out{i}"].view(P.OUT_DTYPE).reshape(-1) for i in (0, 1)),
                         ctr=(d["ctr0"], d["ctr1"]))
    fx.n = fx.geom.shape[0]
    fx.params = SimpleNamespace(spp=fx.spp)
    return fx


def canon(a, fields):
    """A copy of answers with every NaN in the float `fields` replaced by one NaN: IEEE 754 leaves the
    sign and payload of a NaN an operation makes (normalize(0), arithmetic on a NaN direction) to the
    implementation, and the CPU's and the GPU's differ.  Every number, and every other field, keeps its bits."""
    a = a.copy()
    for f in fields:
        v = a[f]
        v[np.isnan(v)] = np.float32(np.nan)
        a[f] = v
    return a


def canon_hits(h):
    return canon(h, ("n", "extra"))


def canon_out(o):
    return canon(o, ("rgb", "depth"))


def first_difference(got, want, cls, names):
    """None, or a message naming the classes that differ and the first differing query."""
    g, w = got.view(np.uint32).reshape(-1, 8), want.view(np.uint32).reshape(-1, 8)
    bad = np.flatnonzero((g != w).any(1))
    if not len(bad):
        return None
    per = {names[c]: int((cls[bad] == c).sum()) for c in np.unique(cls[bad])}
    return (f"{len(bad)} of {len(got)} differ, by class {per}; first {bad[0]} ({names[cls[bad[0]]]}): "
            f"got {got[bad[0]]} want {want[bad[0]]}")
