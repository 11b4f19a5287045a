"""The path-query entry points of the C ABI without a device: the Python mirror's record layouts
match rt_path_ray / rt_path_out, the header declares them, and every argument error of both entry
points comes back before any device is touched."""
import ctypes as C
import os
import re

import numpy as np

import rt_amd as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_record_layouts():
    assert R.PATH_RAY_DTYPE.itemsize == 32 and R.PATH_OUT_DTYPE.itemsize == 32
    assert [R.PATH_RAY_DTYPE.fields[k][1] for k in ("o", "sample", "d", "pad")] == [0, 12, 16, 28]
    assert [R.PATH_OUT_DTYPE.fields[k][1] for k in ("rgb", "depth", "segments", "drops", "nans", "status")] == \
        [0, 12, 16, 20, 24, 28]
    assert R.PATH_RAY_DTYPE["sample"] == np.uint32 and R.PATH_OUT_DTYPE["status"] == np.uint32
    assert R.ABI_VERSION == 5 and R.load().rt_abi_version() == 5


def test_header_declares_the_queries():
    src = open(os.path.join(ROOT, "include", "rt_hip.h")).read()
    assert "typedef struct rt_path_ray { float o[3]; uint32_t sample; float d[3]; uint32_t pad; } rt_path_ray;" in src
    assert ("typedef struct rt_path_out { float rgb[3]; float depth; uint32_t segments, drops, nans, status; } "
            "rt_path_out;") in src
    assert re.search(r"#define\s+RT_ABI_VERSION\s+5\b", src)
    assert src.index("rt_trace_iow03(") < src.index("rt_path_rays_async(") < src.index("rt_path_inw(")
    dbg = open(os.path.join(ROOT, "include", "rt_hip_debug.h")).read()
    assert "int rt_debug_paths_kernel(int lights, int fused, int info[4]);" in dbg
    assert "int rt_debug_paths_max_blocks(int blocks);" in dbg
    for name in ("rt_path_rays_async", "rt_path_inw", "rt_debug_paths_kernel", "rt_debug_paths_max_blocks"):
        assert name in R.SIGNATURES and hasattr(R.load(), name)
    # why IOW-03 scenes are refused, and what depth is
    assert re.search(r"RT_E_UNSUPPORTED for an IOW-03 scene: an IOW-03 sample reads the RI stack", src)
    assert "not a hit distance" in src


def test_async_argument_errors():
    lib = R.load()
    buf = np.zeros(8, np.float32)
    p = buf.ctypes.data
    assert lib.rt_path_rays_async(None, p, 1, 8, 0, p, None, None) == R.RT_E_ARG
    assert lib.rt_path_rays_async(None, None, 0, 8, 0, None, None, None) == R.RT_E_ARG  # null scene, even for no rays
    assert lib.rt_path_rays_async(None, p, 1, -1, 0, p, None, None) == R.RT_E_ARG
    assert lib.rt_path_rays_async(None, p, 1, 8, R.RT_TRACE_ANY, p, None, None) == R.RT_E_ARG
    assert not buf.any()


def test_blocking_argument_errors():
    lib = R.load()
    geom = np.zeros((1, 28), np.float32)
    nodes = np.zeros((1, 8), np.float32)
    lights = np.zeros((1, 7), np.float32)
    rays = np.zeros(1, R.PATH_RAY_DTYPE)
    out = np.zeros(1, R.PATH_OUT_DTYPE)
    st = R.RtStats()
    texels = np.zeros((2, 2, 3), np.uint8)
    bad_tex = (R.RtTexture * 1)(R.RtTexture(texels.ctypes.data, 2, 0, 3))

    def call(g=geom, n=1, layout=1, nd=nodes, lt=None, nl=0, tex=None, nt=0, spp=4, mb=8, r=rays.ctypes.data, nr=1,
             flags=0, o=out.ctypes.data):
        return lib.rt_path_inw(R.fptr(g), n, layout, R.fptr(nd), R.fptr(lt), nl, tex, nt, spp, mb, r, nr, flags, o, -1,
                               C.byref(st))

    assert call(g=None) == R.RT_E_ARG
    assert call(nd=None) == R.RT_E_ARG
    assert call(n=0) == R.RT_E_ARG
    assert call(layout=3) == R.RT_E_ARG and call(layout=0) == R.RT_E_ARG
    assert call(spp=0) == R.RT_E_ARG and call(spp=-3) == R.RT_E_ARG
    assert call(mb=-1) == R.RT_E_ARG
    assert call(layout=4, lt=None, nl=1) == R.RT_E_ARG          # lights counted but not given
    assert call(layout=4, tex=bad_tex, nt=1) == R.RT_E_ARG      # a texture without rows
    assert call(layout=4, tex=None, nt=1) == R.RT_E_ARG
    assert call(flags=R.RT_TRACE_ANY) == R.RT_E_ARG             # any bit other than RT_TRACE_INVERT
    assert call(flags=R.RT_TRACE_INVERT | 4) == R.RT_E_ARG and call(flags=-1) == R.RT_E_ARG
    assert call(r=None) == R.RT_E_ARG and call(o=None) == R.RT_E_ARG   # null rays / out with n_rays > 0
    assert call(nr=(1 << 31) + 1) == R.RT_E_ARG
    textured = geom.copy()
    textured[0, 27] = 1.0                                        # layout 4: TextureIndex 1, none bound
    assert call(g=textured, layout=4) == R.RT_E_UNSUPPORTED
    assert call(g=textured, layout=4, flags=2) == R.RT_E_ARG     # argument errors come first
    assert call(g=textured, layout=4, lt=lights, nl=1) == R.RT_E_UNSUPPORTED
    assert not out.view(np.uint8).any()
