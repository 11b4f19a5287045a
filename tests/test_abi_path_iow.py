"""The IOW-03 path-query entry points of the C ABI without a device: the Python mirror's record
layouts match rt_path_iow_ray / rt_path_iow_out, the header declares them after the INW path queries,
and every argument error of both entry points comes back before any device is touched, with the
output buffer as the caller left it."""
import ctypes as C
import os
import re

import numpy as np

import rt_amd as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0xA5


def test_record_layouts():
    ray, out = R.PATH_IOW_RAY_DTYPE, R.PATH_IOW_OUT_DTYPE
    assert ray.itemsize == 48 and out.itemsize == 48
    assert [ray.fields[k][1] for k in ("o", "sample", "d", "pad", "ri_in")] == [0, 12, 16, 28, 32]
    assert [out.fields[k][1] for k in ("rgb", "stale", "segments", "drops", "nans", "status", "ri_out")] == \
        [0, 12, 16, 20, 24, 28, 32]
    assert ray["sample"] == np.uint32 and out["stale"] == np.uint32 and out["status"] == np.uint32
    assert ray["ri_in"].shape == (4,) and out["ri_out"].shape == (4,)
    assert R.ABI_VERSION == 5 and R.load().rt_abi_version() == 5


def test_header_declares_the_queries():
    src = open(os.path.join(ROOT, "include", "rt_hip.h")).read()
    assert ("typedef struct rt_path_iow_ray { float o[3]; uint32_t sample; float d[3]; uint32_t pad; float ri_in[4]; } "
            "rt_path_iow_ray;") in src
    assert ("typedef struct rt_path_iow_out { float rgb[3]; uint32_t stale; uint32_t segments, drops, nans, status; "
            "float ri_out[4]; } rt_path_iow_out;") in src
    assert re.search(r"#define\s+RT_ABI_VERSION\s+5\b", src)
    after = src.index("int rt_path_inw(")
    for decl in ("typedef struct rt_path_iow_ray", "typedef struct rt_path_iow_out", "int rt_path_iow_rays_async(",
                 "int rt_path_iow03("):
        assert src.index(decl) > after, decl
    # the INW query still refuses IOW-03 scenes, in the same words
    assert "so a single ray has no defined radiance there" in src
    dbg = open(os.path.join(ROOT, "include", "rt_hip_debug.h")).read()
    for decl in ("int rt_debug_path_iow_kernel(int lds_nodes, int info[4]);",
                 "int rt_debug_path_iow_max_blocks(int blocks);"):
        assert decl in dbg and decl not in src
    assert "rt_debug_path_iow" not in src
    for name in ("rt_path_iow_rays_async", "rt_path_iow03", "rt_debug_path_iow_kernel",
                 "rt_debug_path_iow_max_blocks"):
        assert name in R.SIGNATURES and hasattr(R.load(), name)


def test_async_argument_errors():
    """No scene can exist without a device, and a null scene is an error whatever else is passed."""
    lib = R.load()
    buf = np.full(24, FILL, np.uint8)
    rays = np.zeros(1, R.PATH_IOW_RAY_DTYPE)
    p, r = buf.ctypes.data, rays.ctypes.data
    assert lib.rt_path_iow_rays_async(None, r, 1, 1, 8, 0, p, None, None) == R.RT_E_ARG
    assert lib.rt_path_iow_rays_async(None, None, 0, 1, 8, 0, None, None, None) == R.RT_E_ARG  # even for no rays
    assert lib.rt_path_iow_rays_async(None, r, 1, 0, 8, 0, p, None, None) == R.RT_E_ARG        # chain == 0
    assert lib.rt_path_iow_rays_async(None, r, 1, 1, -1, 0, p, None, None) == R.RT_E_ARG       # max_bounces < 0
    assert lib.rt_path_iow_rays_async(None, r, 1, 1, 8, 1, p, None, None) == R.RT_E_ARG        # flags are reserved
    assert lib.rt_path_iow_rays_async(None, r, (1 << 31) + 1, 1, 8, 0, p, None, None) == R.RT_E_ARG
    assert np.all(buf == FILL)


def test_blocking_argument_errors():
    lib = R.load()
    types = np.full(1, R.RT_IOW_ELLIPSOID, np.float32)
    rec = np.zeros((1, 24), np.float32)
    rays = np.zeros(2, R.PATH_IOW_RAY_DTYPE)
    out = np.full(2 * 48, FILL, np.uint8)
    st = R.RtStats()

    def call(ty=types, rc=rec, n=1, spp=8, mb=8, r=rays.ctypes.data, nr=2, chain=1, flags=0, o=out.ctypes.data):
        return lib.rt_path_iow03(R.fptr(ty), R.fptr(rc), n, spp, mb, r, nr, chain, flags, o, -1, C.byref(st))

    assert call(ty=None) == R.RT_E_ARG and call(rc=None) == R.RT_E_ARG
    assert call(n=0) == R.RT_E_ARG
    assert call(spp=0) == R.RT_E_ARG and call(spp=-3) == R.RT_E_ARG
    assert call(mb=-1) == R.RT_E_ARG
    assert call(chain=0) == R.RT_E_ARG
    assert call(flags=1) == R.RT_E_ARG and call(flags=R.RT_TRACE_ANY) == R.RT_E_ARG and call(flags=-1) == R.RT_E_ARG
    assert call(r=None) == R.RT_E_ARG and call(o=None) == R.RT_E_ARG   # null rays / out with n_rays > 0
    assert call(nr=(1 << 31) + 1) == R.RT_E_ARG
    assert call(nr=0, chain=0) == R.RT_E_ARG and call(nr=0, flags=1) == R.RT_E_ARG  # ... also with nothing to do
    assert np.all(out == FILL)
