"""Builds and calls tests/trace_iow_ref.c, the CPU reference of the IOW-03 ray-query tests: the
oracle's own launch_ray() per query.  Used by tests/golden/make_trace_iow_golden.py (writes the
trace_iow_*.npz fixtures) and tests/test_trace_iow_ref.py (recomputes them)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")

# the trace_iow_*.npz fixtures, in the order the generator writes them
SCENES = ["final", "final2", "ref3", "one", "rot", "dups", "touch", "shells", "chain"]

RAY_DTYPE = np.dtype([("o", np.float32, 3), ("tmax", np.float32), ("d", np.float32, 3), ("ratio", np.float32)])
HIT_DTYPE = np.dtype([("t", np.float32), ("id", np.int32), ("n", np.float32, 3), ("extra", np.float32),
                      ("pad", np.uint32, 2)])


def build(out_dir: str) -> C.CDLL:
    """Compile trace_iow_ref.c (with the oracle's sources, its numerics flags) into out_dir and load it."""
    so = os.path.join(str(out_dir), "libtrace_iow_ref.so")
    orc = os.path.join(ROOT, "oracle")
    subprocess.run(["gcc", "-O2", "-std=c11", "-D_POSIX_C_SOURCE=200809L", "-fPIC", "-fopenmp", "-ffp-contract=off",
                    "-fno-math-errno", "-shared", "-o", so, os.path.join(HERE, "trace_iow_ref.c"),
                    os.path.join(orc, "rt_oracle_host.c"), os.path.join(orc, "rt_oracle_tex.c"), "-lm"], check=True)
    lib = C.CDLL(so)
    lib.trace_iow_ref.restype = C.c_int
    lib.trace_iow_ref.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
    return lib


def run(lib, types, records, rays):
    """hits (HIT_DTYPE); asserts that the reference refused no query."""
    types = np.ascontiguousarray(types, np.float32)
    records = np.ascontiguousarray(records, np.float32)
    rays = np.ascontiguousarray(rays, RAY_DTYPE)
    hits = np.zeros(rays.shape, HIT_DTYPE)
    rc = lib.trace_iow_ref(types.ctypes.data, records.ctypes.data, len(types), rays.ctypes.data, rays.size,
                           hits.ctypes.data)
    assert rc == 0, f"trace_iow_ref refused query {rc - 1}" if rc > 0 else "bad arguments"
    return hits


def load_fixture(name: str) -> dict:
    with np.load(os.path.join(GOLDEN, f"trace_iow_{name}.npz")) as z:
        d = {k: z[k] for k in z.files}
    d["rays"] = d["rays"].view(RAY_DTYPE).reshape(-1)
    d["hits"] = d["hits"].view(HIT_DTYPE).reshape(-1)
    return d


def same_hits(a, b) -> bool:
    """Bit-for-bit: t, id, normal, extra (pad is 0 in both)."""
    return a.shape == b.shape and a.tobytes() == b.tobytes()
