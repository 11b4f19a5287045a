"""The IOW-03 ray-query entry points of the C ABI without a device: the header declares them, the
Python mirror binds them, and every argument error comes back before any device is touched, with the
hit buffer untouched."""
import ctypes as C
import os
import re

import numpy as np

import rt_amd as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_mirror_declare_the_queries():
    src = open(os.path.join(ROOT, "include", "rt_hip.h")).read()
    assert re.search(r"\bint\s+rt_trace_iow_rays_async\s*\(\s*rt_dev_scene\s*\*", src)
    assert re.search(r"\bint\s+rt_trace_iow03\s*\(\s*const\s+float\s*\*\s*types", src)
    assert "rt_debug_trace_iow_kernel" not in src  # debug hooks live in rt_hip_debug.h
    assert "rt_debug_trace_iow_kernel" in open(os.path.join(ROOT, "include", "rt_hip_debug.h")).read()
    assert re.search(r"#define\s+RT_ABI_VERSION\s+5\b", src) and R.ABI_VERSION == 5
    for name in ("rt_trace_iow_rays_async", "rt_trace_iow03"):
        assert name in R.SIGNATURES and hasattr(R.load(), name)
    assert callable(R.trace_iow)


def test_async_argument_errors():
    lib = R.load()
    hits = np.full(8, 0xCDCDCDCD, np.uint32)
    rays = np.zeros(1, R.RAY_DTYPE)
    assert lib.rt_trace_iow_rays_async(None, rays.ctypes.data, 1, 0, hits.ctypes.data, None, None) == R.RT_E_ARG
    assert lib.rt_trace_iow_rays_async(None, None, 0, 0, None, None, None) == R.RT_E_ARG  # null scene, even for no rays
    assert np.all(hits == 0xCDCDCDCD)


def test_blocking_argument_errors():
    lib = R.load()
    types = np.full(1, float(R.RT_IOW_ELLIPSOID), np.float32)
    rec = np.zeros((1, 24), np.float32)
    rec[0, 3:12] = (1, 0, 0, 0, 1, 0, 0, 0, 1)
    rec[0, 12:15] = 1.0
    rays = np.zeros(1, R.RAY_DTYPE)
    hits = np.zeros(1, R.HIT_DTYPE)
    hits.view(np.uint8)[:] = 0xCD
    st = R.RtStats()

    def call(ty=types, rc=rec, n=1, r=rays.ctypes.data, nr=1, flags=0, h=hits.ctypes.data):
        return lib.rt_trace_iow03(R.fptr(ty), R.fptr(rc), n, r, nr, flags, h, -1, C.byref(st))

    assert call(flags=R.RT_TRACE_INVERT) == R.RT_E_ARG  # no meaning on IOW-03
    assert call(flags=R.RT_TRACE_INVERT | R.RT_TRACE_ANY) == R.RT_E_ARG
    assert call(flags=4) == R.RT_E_ARG                   # unknown flag bits
    assert call(flags=-1) == R.RT_E_ARG
    assert call(ty=None) == R.RT_E_ARG
    assert call(rc=None) == R.RT_E_ARG
    assert call(n=0) == R.RT_E_ARG
    assert call(r=None) == R.RT_E_ARG                    # null rays / hits with n_rays > 0
    assert call(h=None) == R.RT_E_ARG
    assert call(nr=2 ** 31 + 1) == R.RT_E_ARG            # more than 2^31 queries
    assert np.all(hits.view(np.uint8) == 0xCD)
