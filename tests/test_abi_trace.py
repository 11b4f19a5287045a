"""The ray-query entry points of the C ABI without a device: the Python mirror's record layouts
match rt_ray / rt_hit, and the argument errors come back before any device is touched."""
import ctypes as C
import os
import re

import numpy as np

import rt_amd as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_record_layouts():
    assert R.RAY_DTYPE.itemsize == 32 and R.HIT_DTYPE.itemsize == 32
    assert [R.RAY_DTYPE.fields[k][1] for k in ("o", "tmax", "d", "ratio")] == [0, 12, 16, 28]
    assert [R.HIT_DTYPE.fields[k][1] for k in ("t", "id", "n", "extra", "pad")] == [0, 4, 8, 20, 24]
    assert (R.RT_TRACE_INVERT, R.RT_TRACE_ANY) == (1, 2)


def test_header_declares_the_queries():
    src = open(os.path.join(ROOT, "include", "rt_hip.h")).read()
    assert re.search(r"#define\s+RT_TRACE_INVERT\s+1\b", src) and re.search(r"#define\s+RT_TRACE_ANY\s+2\b", src)
    assert "typedef struct rt_ray { float o[3]; float tmax; float d[3]; float ratio; } rt_ray;" in src
    assert "typedef struct rt_hit { float t; int32_t id; float n[3]; float extra; uint32_t pad[2]; } rt_hit;" in src
    for name in ("rt_trace_rays_async", "rt_trace_inw"):
        assert name in R.SIGNATURES and hasattr(R.load(), name)


def test_async_argument_errors():
    lib = R.load()
    buf = np.zeros(8, np.float32)
    p = buf.ctypes.data
    assert lib.rt_trace_rays_async(None, p, 1, 0, p, None, None) == R.RT_E_ARG
    assert lib.rt_trace_rays_async(None, None, 0, 0, None, None, None) == R.RT_E_ARG  # null scene, even for no rays


def test_blocking_argument_errors():
    lib = R.load()
    geom = np.zeros((1, 28), np.float32)
    nodes = np.zeros((1, 8), np.float32)
    rays = np.zeros(1, R.RAY_DTYPE)
    hits = np.zeros(1, R.HIT_DTYPE)
    st = R.RtStats()

    def call(g=geom, n=1, layout=1, nd=nodes, r=rays.ctypes.data, nr=1, flags=0, h=hits.ctypes.data):
        return lib.rt_trace_inw(R.fptr(g), n, layout, R.fptr(nd), r, nr, flags, h, -1, C.byref(st))

    assert call(layout=3) == R.RT_E_ARG        # bad layout
    assert call(layout=0) == R.RT_E_ARG
    assert call(flags=4) == R.RT_E_ARG         # unknown flag bits
    assert call(flags=R.RT_TRACE_INVERT | R.RT_TRACE_ANY | 8) == R.RT_E_ARG
    assert call(flags=-1) == R.RT_E_ARG
    assert call(g=None) == R.RT_E_ARG
    assert call(nd=None) == R.RT_E_ARG
    assert call(n=0) == R.RT_E_ARG
    assert call(r=None) == R.RT_E_ARG          # null rays / hits with n_rays > 0
    assert call(h=None) == R.RT_E_ARG
    assert not hits.view(np.uint8).any()
