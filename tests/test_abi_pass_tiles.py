"""The progressive passes on packed tile lists and device groups (rt_render_pass_tiles_async,
rt_render_pass_multi_async, rt_render_passes_inw_multi) without a device: the library exports them and the
Python mirror declares them, the header declares them in its multi-GPU section, the ABI version and
rt_options are unchanged, and every argument error that needs no scene comes back as RT_E_ARG with the
host buffers untouched.  (The errors that need a scene or a group are in tests/test_gpu_pass_tiles.py and
tests/test_gpu_pass_multi.py.)"""
import ctypes as C
import os
import re

import numpy as np

import rt_amd as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rt_render_pass_tiles_async", "rt_render_pass_multi_async", "rt_render_passes_inw_multi")


def test_exported_and_mirrored():
    lib = R.load()
    for name in NAMES:
        assert name in R.SIGNATURES and hasattr(lib, name), name
    for name in ("render_pass_tiles", "render_passes_multi", "PASS_TILE_KERNELS"):
        assert hasattr(R, name), name
    assert sorted(R.PASS_TILE_KERNELS) == [16, 17, 18, 19]
    assert R.ABI_VERSION == 5 and lib.rt_abi_version() == 5   # additive: the version stays
    assert C.sizeof(R.RtOptions) == R.default_options().size  # rt_options is unchanged


def test_header_declares_them_in_the_multi_gpu_section():
    src = open(os.path.join(ROOT, "include", "rt_hip.h")).read()
    assert re.search(r"#define\s+RT_ABI_VERSION\s+5\b", src)
    assert src.index("rt_render_inw_multi(") < src.index("rt_render_pass_tiles_async(") < \
        src.index("rt_render_pass_multi_async(") < src.index("rt_render_passes_inw_multi(") < src.index("rt_tile_spiral(")
    flat = " ".join(src.split())
    for phrase in ("rt_pass_state *d_state_packed /* n_tiles*T*T */", "slot = tile * T*T + iy * T + ix",
                   "neither read nor written; its image slot is written as (0, 0, 0, 0)", "n_tiles * T*T > 2^31",
                   "fold state never leaves its device", "s0 must be 0 (a new frame) or exactly that count",
                   "A changed deal resets the count to 0", "tile lists and on groups"):
        assert phrase in flat, phrase
    assert "Not covered: packed tile lists" not in flat
    dbg = " ".join(open(os.path.join(ROOT, "include", "rt_hip_debug.h")).read().split())
    assert "which = 16 is k_pass_rays, 17 k_pass_fold" in dbg


def test_tile_pass_argument_errors():
    """No scene exists without a device, so every call here has a null scene or, besides, one more bad
    argument: each is RT_E_ARG before any pointer is read or written."""
    lib = R.load()
    cam, p = R.RtCamera(), R.RtParams(width=16, height=9, spp=4, max_bounces=8)
    buf = np.full(16 * 16 * 8, 7.0, np.float32)
    want = buf.copy()
    b = buf.ctypes.data
    tiles = np.zeros(2, np.int32)
    t = tiles.ctypes.data

    def call(s=None, c=cam, q=p, tl=t, n=1, T=16, s0=0, ns=4, state=b):
        return lib.rt_render_pass_tiles_async(s, C.byref(c) if c is not None else None,
                                              C.byref(q) if q is not None else None, tl, n, T, s0, ns, state, b, b, b, None)

    assert call() == R.RT_E_ARG                                        # null scene
    assert call(c=None) == R.RT_E_ARG and call(q=None) == R.RT_E_ARG   # null cam / p
    assert call(state=None) == R.RT_E_ARG and call(tl=None) == R.RT_E_ARG
    for n in (0, -1):
        assert call(n=n) == R.RT_E_ARG, n
    for T in (0, 8, 24, -16):
        assert call(T=T) == R.RT_E_ARG, T
    for s0 in (4, 5, 0xFFFFFFFF):                                      # s0 >= spp
        assert call(s0=s0) == R.RT_E_ARG, s0
    assert call(n=1 << 23, T=32) == R.RT_E_ARG                         # 2^33 slots
    assert buf.tobytes() == want.tobytes() and not tiles.any()
    info = (C.c_int * 4)()
    for which in (4, 5, 6, 7, 15, 20):
        assert lib.rt_debug_pass_kernel(which, info) == R.RT_E_ARG, which
    assert lib.rt_debug_pass_kernel(16, None) == R.RT_E_ARG


def test_group_pass_argument_errors():
    lib = R.load()
    cam, p = R.RtCamera(), R.RtParams(width=16, height=9, spp=4, max_bounces=8)
    buf = np.full(16 * 9 * 4, 7.0, np.float32)
    want = buf.copy()
    b = buf.ctypes.data
    scenes = (C.c_void_p * 1)(None)
    for s0, ns, T in ((0, 4, 16), (2, 1, 16), (4, 1, 16), (0, 4, 8), (0, 0, 16)):
        assert lib.rt_render_pass_multi_async(None, scenes, C.byref(cam), C.byref(p), T, s0, ns, b, b, b, None) == R.RT_E_ARG
    assert lib.rt_render_pass_multi_async(None, None, None, None, 16, 0, 1, None, None, None, None) == R.RT_E_ARG
    assert buf.tobytes() == want.tobytes()


def test_blocking_group_argument_errors():
    lib = R.load()
    geom = np.zeros((1, 28), np.float32)
    nodes = np.zeros((1, 8), np.float32)
    npx = 16 * 9
    rgba = np.full((2, npx, 4), 3.0, np.float32)
    depth = np.full((2, npx), 3.0, np.float32)
    cam = R.RtCamera()
    st = R.RtStats()
    devs = (C.c_int * 1)(0)

    def params(**kw):
        d = dict(width=16, height=9, spp=4, max_bounces=8)
        d.update(kw)
        return R.RtParams(**d)

    def call(g=geom, n=1, layout=1, nd=nodes, lt=None, nl=0, c=cam, p=None, dv=devs, n_dev=1, T=16, cuts=(2, 4), o=rgba):
        p = params() if p is None else p
        a = None if cuts is None else (C.c_uint32 * max(1, len(cuts)))(*cuts)
        return lib.rt_render_passes_inw_multi(R.fptr(g), n, layout, R.fptr(nd), R.fptr(lt), nl,
                                              C.byref(c) if c is not None else None,
                                              C.byref(p) if p is not False else None, dv, n_dev, T, a,
                                              2 if cuts is None else len(cuts),
                                              R.fptr(o.reshape(-1)) if o is not None else None,
                                              R.fptr(depth.reshape(-1)), C.byref(st))

    assert call(g=None) == R.RT_E_ARG and call(nd=None) == R.RT_E_ARG and call(n=0) == R.RT_E_ARG
    assert call(c=None) == R.RT_E_ARG and call(p=False) == R.RT_E_ARG and call(o=None) == R.RT_E_ARG
    assert call(dv=None) == R.RT_E_ARG and call(n_dev=0) == R.RT_E_ARG
    assert call(layout=3) == R.RT_E_ARG and call(layout=4, nl=1) == R.RT_E_ARG
    for bad in (dict(width=0), dict(height=-1), dict(spp=0)):
        assert call(p=params(**bad)) == R.RT_E_ARG, bad
    for T in (0, 8, 24):
        assert call(T=T) == R.RT_E_ARG, T
    # cuts: null, none, starting at 0, not increasing, decreasing, past spp
    for bad in (None, (), (0, 4), (2, 2), (3, 2), (2, 5), (5,)):
        assert call(cuts=bad) == R.RT_E_ARG, bad
    assert call(p=params(show_normal=1)) == R.RT_E_UNSUPPORTED
    assert call(p=params(show_normal=1), cuts=(0, 4)) == R.RT_E_ARG   # argument errors come first
    assert np.all(rgba == 3.0) and np.all(depth == 3.0)
    assert st.segments == 0 and st.ms == 0.0
