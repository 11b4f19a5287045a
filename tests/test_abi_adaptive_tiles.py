"""The adaptive passes on packed tile lists and device groups (rt_render_pass_slots_async,
rt_pass_select_tiles_async, rt_render_adaptive_multi_async, rt_group_adaptive_active,
rt_render_adaptive_inw_multi) without a device: the library exports them and the Python mirror declares them,
the header holds the contract, the ABI version and rt_options are unchanged, and every argument error that
needs no scene comes back as RT_E_ARG with the host buffers untouched.  (The errors that need a scene or a
group are in tests/test_gpu_adaptive_tiles.py and tests/test_gpu_adaptive_multi.py.)"""
import ctypes as C
import os
import re

import numpy as np

import rt_amd as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rt_render_pass_slots_async", "rt_pass_select_tiles_async", "rt_render_adaptive_multi_async",
         "rt_group_adaptive_active", "rt_render_adaptive_inw_multi")


def test_exported_and_mirrored():
    lib = R.load()
    for name in NAMES:
        assert name in R.SIGNATURES and hasattr(lib, name), name
    for name in ("pass_slots", "pass_select_tiles", "render_adaptive_multi_round", "group_adaptive_active",
                 "render_adaptive_multi", "ADAPTIVE_TILE_KERNELS", "SLOT_NONE"):
        assert hasattr(R, name), name
    assert sorted(R.ADAPTIVE_TILE_KERNELS) == [24, 25, 26, 27, 28, 30] and R.SLOT_NONE == 0xFFFFFFFF
    assert R.ABI_VERSION == 5 and lib.rt_abi_version() == 5   # additive: the version stays
    assert C.sizeof(R.RtOptions) == R.default_options().size  # rt_options is unchanged


def test_header_declares_them_in_the_multi_gpu_section():
    src = open(os.path.join(ROOT, "include", "rt_hip.h")).read()
    assert re.search(r"#define\s+RT_ABI_VERSION\s+5\b", src)
    assert re.search(r"#define\s+RT_SLOT_NONE\s+0xffffffffu\b", src)
    assert src.index("int rt_render_passes_inw_multi(") < src.index("int rt_render_pass_slots_async(") < \
        src.index("int rt_pass_select_tiles_async(") < src.index("int rt_render_adaptive_multi_async(") < \
        src.index("int rt_group_adaptive_active(") < src.index("int rt_render_adaptive_inw_multi(") < \
        src.index("rt_tile_spiral(")
    flat = " ".join(src.split())
    for phrase in ("slot = tile * T*T + iy * T + ix", "[c, min(c + ns, S))", "not read when c == 0",
                   "acc * RN(1 / c')", "Unlisted slots keep every byte", "The list holds no slot twice",
                   "48 is legal", "n_slots > 2^31", "n_slots == 0 or ns == 0 returns RT_OK",
                   "tile-major, 8x8 blocks row-major inside a tile", "THIS CALL BLOCKS",
                   "an rt_render_pass_multi_async pass ran since", "fold state does not leave its device"):
        assert phrase in flat, phrase
    assert "stay uncovered" not in flat
    dbg = " ".join(open(os.path.join(ROOT, "include", "rt_hip_debug.h")).read().split())
    assert "which = 24 is k_adapt_rays, 25 k_adapt_fold" in dbg


def test_slot_pass_and_tile_select_argument_errors():
    """No scene exists without a device, so every call here has a null scene or, besides, one more bad
    argument: each is RT_E_ARG before any pointer is read or written."""
    lib = R.load()
    cam, p = R.RtCamera(), R.RtParams(width=16, height=9, spp=4, max_bounces=8)
    buf = np.full(16 * 16 * 8, 7.0, np.float32)
    want = buf.copy()
    b = buf.ctypes.data
    tiles = np.zeros(2, np.int32)
    t = tiles.ctypes.data

    def slots(s=None, c=cam, q=p, tl=t, n=1, T=16, sl=b, n_slots=4, ns=4, state=b, aux=b):
        return lib.rt_render_pass_slots_async(s, C.byref(c) if c is not None else None,
                                              C.byref(q) if q is not None else None, tl, n, T, sl, n_slots, ns, state,
                                              aux, b, b, b, None)

    def select(s=None, q=p, tl=t, n=1, T=16, state=b, aux=b, tol=0.5, sl=b, na=b):
        return lib.rt_pass_select_tiles_async(s, C.byref(q) if q is not None else None, tl, n, T, state, aux, tol, 2,
                                              sl, na, b, None)

    assert slots() == R.RT_E_ARG and select() == R.RT_E_ARG               # null scene
    assert slots(c=None) == R.RT_E_ARG and slots(q=None) == R.RT_E_ARG and select(q=None) == R.RT_E_ARG
    for call in (slots, select):
        assert call(state=None) == R.RT_E_ARG and call(aux=None) == R.RT_E_ARG and call(tl=None) == R.RT_E_ARG
        for n in (0, -1):
            assert call(n=n) == R.RT_E_ARG, n
        for T in (0, 8, 24, -16):
            assert call(T=T) == R.RT_E_ARG, T
        assert call(n=1 << 23, T=32) == R.RT_E_ARG                        # 2^33 slots
        assert call(n=(1 << 21) + 1, T=32) == R.RT_E_ARG                  # just past 2^31
    assert slots(sl=None) == R.RT_E_ARG and slots(sl=None, n_slots=0) == R.RT_E_ARG
    for n_slots, ns in ((0, 4), (4, 0), (0, 0), ((1 << 31) + 1, 1), (0xFFFFFFFF, 1), (1, 0xFFFFFFFF)):
        assert slots(n_slots=n_slots, ns=ns) == R.RT_E_ARG, (n_slots, ns)
    assert select(sl=None) == R.RT_E_ARG and select(na=None) == R.RT_E_ARG
    for tol in (-1.0, float("nan")):
        assert select(tol=tol) == R.RT_E_ARG
    assert buf.tobytes() == want.tobytes() and not tiles.any()
    info = (C.c_int * 4)()
    for which in (20, 21, 22, 23, 29, 31, 100):   # the tile-list adaptive kernels are 24..28 and 30
        assert lib.rt_debug_pass_kernel(which, info) == R.RT_E_ARG, which
    assert lib.rt_debug_pass_kernel(24, None) == R.RT_E_ARG


def test_group_round_argument_errors():
    lib = R.load()
    cam, p = R.RtCamera(), R.RtParams(width=16, height=9, spp=4, max_bounces=8)
    buf = np.full(16 * 9 * 4, 7.0, np.float32)
    want = buf.copy()
    b = buf.ctypes.data
    scenes = (C.c_void_p * 1)(None)
    for first, ns, T in ((1, 2, 16), (0, 2, 16), (1, 0, 16), (1, 2, 8), (1, 2, 0)):
        assert lib.rt_render_adaptive_multi_async(None, scenes, C.byref(cam), C.byref(p), T, first, ns, 0.1, 2, b, b, b,
                                                  b, None) == R.RT_E_ARG
    assert lib.rt_render_adaptive_multi_async(None, None, None, None, 16, 1, 1, 0.0, 0, None, None, None, None,
                                              None) == R.RT_E_ARG
    n = C.c_uint32(77)
    assert lib.rt_group_adaptive_active(None, C.byref(n)) == R.RT_E_ARG and n.value == 77
    assert buf.tobytes() == want.tobytes()


def test_blocking_group_argument_errors():
    lib = R.load()
    geom = np.zeros((1, 28), np.float32)
    nodes = np.zeros((1, 8), np.float32)
    npx = 16 * 9
    rgba = np.full((npx, 4), 3.0, np.float32)
    depth = np.full(npx, 3.0, np.float32)
    count = np.full(npx, 0xCDCDCDCD, np.uint32)
    rounds = C.c_uint32(77)
    cam = R.RtCamera()
    st = R.RtStats()
    devs = (C.c_int * 1)(0)

    def params(**kw):
        d = dict(width=16, height=9, spp=4, max_bounces=8)
        d.update(kw)
        return R.RtParams(**d)

    def call(g=geom, n=1, layout=1, nd=nodes, lt=None, nl=0, c=cam, p=None, dv=devs, n_dev=1, T=16, batch=2, o=rgba):
        p = params() if p is None else p
        return lib.rt_render_adaptive_inw_multi(R.fptr(g), n, layout, R.fptr(nd), R.fptr(lt), nl,
                                                C.byref(c) if c is not None else None,
                                                C.byref(p) if p is not False else None, dv, n_dev, T, batch, 0.1, 2, 0,
                                                R.fptr(o.reshape(-1)) if o is not None else None, R.fptr(depth),
                                                count.ctypes.data, C.addressof(rounds), C.byref(st))

    assert call(g=None) == R.RT_E_ARG and call(nd=None) == R.RT_E_ARG and call(n=0) == R.RT_E_ARG
    assert call(c=None) == R.RT_E_ARG and call(p=False) == R.RT_E_ARG and call(o=None) == R.RT_E_ARG
    assert call(dv=None) == R.RT_E_ARG and call(n_dev=0) == R.RT_E_ARG and call(batch=0) == R.RT_E_ARG
    assert call(layout=3) == R.RT_E_ARG and call(layout=4, nl=1) == R.RT_E_ARG
    for bad in (dict(width=0), dict(height=-1), dict(spp=0), dict(max_bounces=-1)):
        assert call(p=params(**bad)) == R.RT_E_ARG, bad
    for T in (0, 8, 24):
        assert call(T=T) == R.RT_E_ARG, T
    assert call(p=params(show_normal=1)) == R.RT_E_UNSUPPORTED
    assert call(p=params(show_normal=1), batch=0) == R.RT_E_ARG   # argument errors come first
    assert np.all(rgba == 3.0) and np.all(depth == 3.0) and np.all(count == 0xCDCDCDCD)
    assert rounds.value == 77 and st.segments == 0 and st.ms == 0.0
