"""Builds and calls tests/trace_ref.c, the CPU reference of the ray-query tests: the oracle's own
closest-hit walk per query.  Used by tests/golden/make_trace_golden.py (writes the trace_*.npz
fixtures) and tests/test_trace_ref.py (recomputes them)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")

# the trace_*.npz fixtures, in the order the generator writes them
SCENES = ["spheres1500", "spheres1500_b", "mixed700", "one", "three", "dups300", "pile120", "refset4",
          "shrunk06", "shrunk09"]

RAY_DTYPE = np.dtype([("o", np.float32, 3), ("tmax", np.float32), ("d", np.float32, 3), ("ratio", np.float32)])
HIT_DTYPE = np.dtype([("t", np.float32), ("id", np.int32), ("n", np.float32, 3), ("extra", np.float32),
                      ("pad", np.uint32, 2)])


def build(out_dir: str) -> C.CDLL:
    """Compile trace_ref.c (with the oracle's sources, its numerics flags) into out_dir and load it."""
    so = os.path.join(str(out_dir), "libtrace_ref.so")
    orc = os.path.join(ROOT, "oracle")
    subprocess.run(["gcc", "-O2", "-std=c11", "-D_POSIX_C_SOURCE=200809L", "-fPIC", "-fopenmp", "-ffp-contract=off",
                    "-fno-math-errno", "-shared", "-o", so, os.path.join(HERE, "trace_ref.c"),
                    os.path.join(orc, "rt_oracle_host.c"), os.path.join(orc, "rt_oracle_tex.c"), "-lm"], check=True)
    lib = C.CDLL(so)
    lib.trace_ref.restype = C.c_int
    lib.trace_ref.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p,
                              C.c_void_p]
    return lib


def run(lib, geom, nodes, layout, rays, invert):
    """(hits (HIT_DTYPE), counters uint64[3] = node visits, primitive tests, dropped pushes)."""
    geom = np.ascontiguousarray(geom, np.float32)
    nodes = np.ascontiguousarray(nodes, np.float32)
    rays = np.ascontiguousarray(rays, RAY_DTYPE)
    hits = np.zeros(rays.shape, HIT_DTYPE)
    ctr = np.zeros(3, np.uint64)
    rc = lib.trace_ref(geom.ctypes.data, geom.shape[0], int(layout), nodes.ctypes.data, rays.ctypes.data, rays.size,
                       int(invert), hits.ctypes.data, ctr.ctypes.data)
    assert rc == 0, rc
    return hits, ctr


def load_fixture(name: str) -> dict:
    with np.load(os.path.join(GOLDEN, f"trace_{name}.npz")) as z:
        d = {k: z[k] for k in z.files}
    d["rays"] = d["rays"].view(RAY_DTYPE).reshape(-1)
    for k in ("hits0", "hits1"):
        d[k] = d[k].view(HIT_DTYPE).reshape(-1)
    d["layout"] = int(d["layout"])
    return d


def same_hits(a, b) -> bool:
    """Bit-for-bit: t, id, normal, extra (pad is 0 in both)."""
    return a.shape == b.shape and a.tobytes() == b.tobytes()
