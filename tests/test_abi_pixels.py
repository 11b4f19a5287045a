"""The pixel-query entry points of the C ABI without a device: the library exports them and the Python
mirror declares them, the record layouts match rt_pixel / rt_pixel_out, the header holds the contract,
and every argument error comes back before any device is touched.  (rt_pixel_workspace_bytes of a
scene needs a device to make the scene: tests/test_gpu_pixels.py checks its size with every query.)"""
import ctypes as C
import os
import re

import numpy as np

import rt_amd as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rt_camera_rays_async", "rt_pixel_workspace_bytes", "rt_pixel_query_async", "rt_pixels_inw",
         "rt_pixels_iow03", "rt_debug_pixels_kernel")


def test_exported_and_mirrored():
    lib = R.load()
    for name in NAMES:
        assert name in R.SIGNATURES and hasattr(lib, name), name
    for name in ("camera_rays", "pixels", "pixels_kernel_info", "PIXEL_DTYPE", "PIXEL_OUT_DTYPE"):
        assert hasattr(R, name), name
    assert R.ABI_VERSION == 5 and lib.rt_abi_version() == 5  # additive: the version stays


def test_record_layouts():
    assert R.PIXEL_DTYPE.itemsize == 8 and R.PIXEL_OUT_DTYPE.itemsize == 32
    assert [R.PIXEL_DTYPE.fields[k][1] for k in ("x", "y")] == [0, 4]
    assert R.PIXEL_DTYPE["x"] == np.int32 and R.PIXEL_DTYPE["y"] == np.int32
    assert [R.PIXEL_OUT_DTYPE.fields[k][1] for k in ("rgba", "depth", "segments", "drops", "nans")] == \
        [0, 16, 20, 24, 28]
    px = R.as_pixels([(3, 4), (-1, 7)])
    assert px.dtype == R.PIXEL_DTYPE and px.tobytes() == np.array([3, 4, -1, 7], np.int32).tobytes()


def test_header_declares_the_queries():
    src = open(os.path.join(ROOT, "include", "rt_hip.h")).read()
    assert "typedef struct rt_pixel { int32_t x, y; } rt_pixel;" in src
    assert ("typedef struct rt_pixel_out { float rgba[4]; float depth; uint32_t segments, drops, nans; } "
            "rt_pixel_out;") in src
    assert re.search(r"#define\s+RT_ABI_VERSION\s+5\b", src)
    assert src.index("rt_path_iow03(") < src.index("rt_camera_rays_async(") < src.index("rt_pixel_query_async(") < \
        src.index("rt_pixels_inw(") < src.index("rt_pixels_iow03(")
    assert "size_t rt_pixel_workspace_bytes(const rt_dev_scene *s, uint32_t n_pixels);" in src
    dbg = open(os.path.join(ROOT, "include", "rt_hip_debug.h")).read()
    assert "int rt_debug_pixels_kernel(int which, int info[4]);" in dbg


def test_async_argument_errors():
    """A null scene is an error whatever else is passed, before any pointer is read or written."""
    lib = R.load()
    cam, p = R.RtCamera(), R.RtParams(width=16, height=9, spp=4, max_bounces=8)
    buf = np.zeros(64, np.float32)
    b = buf.ctypes.data
    for n_pixels, ns in ((1, 1), (0, 1), (1, 0), (1 << 16, 1 << 16)):
        assert lib.rt_camera_rays_async(None, C.byref(cam), C.byref(p), b, n_pixels, 0, ns, b, None) == R.RT_E_ARG
    assert lib.rt_camera_rays_async(None, None, None, None, 1, 0, 1, None, None) == R.RT_E_ARG
    for n_pixels in (1, 0, 1 << 30):
        assert lib.rt_pixel_query_async(None, C.byref(cam), C.byref(p), b, n_pixels, b, None, b, 1 << 40, None,
                                        None) == R.RT_E_ARG
    assert lib.rt_pixel_query_async(None, None, None, None, 1, None, None, None, 0, None, None) == R.RT_E_ARG
    assert lib.rt_pixel_workspace_bytes(None, 5) == 0
    assert lib.rt_debug_pixels_kernel(0, None) == R.RT_E_ARG
    info = (C.c_int * 4)()
    assert lib.rt_debug_pixels_kernel(4, info) == R.RT_E_ARG and lib.rt_debug_pixels_kernel(-1, info) == R.RT_E_ARG
    assert not buf.any()


def test_blocking_argument_errors():
    lib = R.load()
    geom = np.zeros((1, 28), np.float32)
    nodes = np.zeros((1, 8), np.float32)
    types = np.zeros(1, np.float32)
    rec = np.zeros((1, 24), np.float32)
    px = np.zeros(2, R.PIXEL_DTYPE)
    out = np.zeros(2, R.PIXEL_OUT_DTYPE)
    cam = R.RtCamera()
    st = R.RtStats()
    texels = np.zeros((2, 2, 3), np.uint8)
    bad_tex = (R.RtTexture * 1)(R.RtTexture(texels.ctypes.data, 2, 0, 3))

    def params(**kw):
        d = dict(width=16, height=9, spp=4, max_bounces=8)
        d.update(kw)
        return R.RtParams(**d)

    def inw(g=geom, n=1, layout=1, nd=nodes, lt=None, nl=0, tex=None, nt=0, c=cam, p=None, x=px.ctypes.data, npx=2,
            o=out.ctypes.data):
        p = params() if p is None else p
        return lib.rt_pixels_inw(R.fptr(g), n, layout, R.fptr(nd), R.fptr(lt), nl, tex, nt,
                                 C.byref(c) if c is not None else None, C.byref(p) if p is not False else None,
                                 x, npx, None, None, o, -1, C.byref(st))

    def iow(t=types, r=rec, n=1, c=cam, p=None, x=px.ctypes.data, npx=2, o=out.ctypes.data):
        p = params() if p is None else p
        return lib.rt_pixels_iow03(R.fptr(t), R.fptr(r), n, C.byref(c) if c is not None else None,
                                   C.byref(p) if p is not False else None, x, npx, None, None, o, -1, C.byref(st))

    for call in (inw, iow):
        assert call(c=None) == R.RT_E_ARG and call(p=False) == R.RT_E_ARG       # null cam / params
        assert call(n=0) == R.RT_E_ARG
        for bad in (dict(width=0), dict(height=-1), dict(spp=0), dict(max_bounces=-1)):
            assert call(p=params(**bad)) == R.RT_E_ARG, bad
        assert call(x=None) == R.RT_E_ARG and call(o=None) == R.RT_E_ARG        # null pixels / out with n_pixels > 0
        assert call(p=params(spp=1 << 16), npx=(1 << 15) + 1) == R.RT_E_ARG    # n_pixels * spp > 2^31
        assert call(p=params(show_normal=1)) == R.RT_E_UNSUPPORTED              # that mode is not a path
        assert call(p=params(show_normal=1), x=None) == R.RT_E_ARG             # argument errors come first
    assert inw(g=None) == R.RT_E_ARG and inw(nd=None) == R.RT_E_ARG
    assert inw(layout=3) == R.RT_E_ARG and inw(layout=0) == R.RT_E_ARG
    assert inw(layout=4, lt=None, nl=1) == R.RT_E_ARG                           # lights counted but not given
    assert inw(layout=4, tex=bad_tex, nt=1) == R.RT_E_ARG                       # a texture without rows
    textured = geom.copy()
    textured[0, 27] = 1.0                                                       # layout 4: TextureIndex 1, none bound
    assert inw(g=textured, layout=4) == R.RT_E_UNSUPPORTED
    assert iow(t=None) == R.RT_E_ARG and iow(r=None) == R.RT_E_ARG
    assert not out.view(np.uint8).any()
