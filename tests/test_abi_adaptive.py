"""The adaptive-pass entry points of the C ABI without a device: the library exports them and the Python
mirror declares them, rt_pass_aux has its stated layout, the header holds the contract, and every argument
error that needs no scene comes back before any device is touched, with the buffers untouched.  (What needs
a scene -- another spp, the null buffers behind a valid scene, show_normal, and RT_OK for n_pixels == 0 or
ns == 0 -- is in tests/test_gpu_adaptive.py.)"""
import ctypes as C
import os
import re

import numpy as np

import rt_amd as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rt_render_pass_pixels_async", "rt_pass_select_async", "rt_render_adaptive_inw", "rt_render_adaptive_iow03",
         "rt_debug_adaptive_chunk")


def test_exported_and_mirrored():
    lib = R.load()
    for name in NAMES:
        assert name in R.SIGNATURES and hasattr(lib, name), name
    for name in ("render_adaptive", "pass_select", "pass_pixels", "PASS_AUX_DTYPE", "ADAPTIVE_KERNELS"):
        assert hasattr(R, name), name
    assert R.ABI_VERSION == 5 and lib.rt_abi_version() == 5  # additive: the version stays
    assert C.sizeof(R.RtOptions) == R.default_options().size    # rt_options is unchanged


def test_aux_layout():
    d = R.PASS_AUX_DTYPE
    assert d.itemsize == 16
    assert [d.fields[k][1] for k in ("even", "count")] == [0, 12]
    assert d["even"].shape == (3,) and d["even"].base == np.float32 and d["count"] == np.uint32
    assert R.PIXEL_DTYPE.itemsize == 8


def test_header_declares_the_adaptive_passes():
    src = open(os.path.join(ROOT, "include", "rt_hip.h")).read()
    assert "typedef struct rt_pass_aux { float even[3]; uint32_t count; } rt_pass_aux;" in src
    assert re.search(r"#define\s+RT_ABI_VERSION\s+5\b", src)
    assert src.index("rt_render_passes_iow03(") < src.index("int rt_render_pass_pixels_async(") < \
        src.index("int rt_pass_select_async(") < src.index("int rt_render_adaptive_inw(") < \
        src.index("int rt_render_adaptive_iow03(") < src.index("rt_tile_deal(")
    flat = " ".join(src.split())
    for phrase in ("[c, min(c + ns, S))", "not read when c == 0", "acc * RN(1 / c')", "Unlisted pixels keep every byte",
                   "is skipped", "{-1, -1}", "p->tile_* is ignored", "n_pixels == 0 or ns == 0 returns RT_OK",
                   "err = (|a.x - e.x| + |a.y - e.y|) + |a.z - e.z|", "err = +inf for n < 2",
                   "n < S && (n < min_samples || !(err <= tol))", "graph-capturable",
                   "served by rt_render_pass_pixels_async"):
        assert phrase in flat, phrase
    dbg = open(os.path.join(ROOT, "include", "rt_hip_debug.h")).read()
    assert "int rt_debug_adaptive_chunk(int samples);" in dbg


def test_async_argument_errors():
    """A null scene is an error whatever else is passed, before any pointer is read or written."""
    lib = R.load()
    cam, p = R.RtCamera(), R.RtParams(width=16, height=9, spp=4, max_bounces=8)
    buf = np.full(64, 7.0, np.float32)
    want = buf.copy()
    b = buf.ctypes.data
    for n_pixels, ns in ((4, 4), (0, 4), (4, 0), (0, 0), (0xFFFFFFFF, 1), (1, 0xFFFFFFFF)):
        assert lib.rt_render_pass_pixels_async(None, C.byref(cam), C.byref(p), b, n_pixels, ns, b, b, b, b, b,
                                               None) == R.RT_E_ARG
    assert lib.rt_render_pass_pixels_async(None, None, None, None, 1, 1, None, None, None, None, None,
                                           None) == R.RT_E_ARG
    for tol in (0.5, -1.0, float("nan")):
        assert lib.rt_pass_select_async(None, C.byref(p), b, b, tol, 2, b, b, b, None) == R.RT_E_ARG
    assert lib.rt_pass_select_async(None, None, None, None, 0.0, 0, None, None, None, None) == R.RT_E_ARG
    info = (C.c_int * 4)()
    for which in (-1, 4, 5, 6, 7, 15, 100):   # the adaptive kernels are 8..14; 4..7 stay errors
        assert lib.rt_debug_pass_kernel(which, info) == R.RT_E_ARG, which
    assert lib.rt_debug_pass_kernel(8, None) == R.RT_E_ARG
    prev = lib.rt_debug_adaptive_chunk(3)
    assert lib.rt_debug_adaptive_chunk(-5) == 3 and lib.rt_debug_adaptive_chunk(prev) == 0  # negative: no cap
    assert lib.rt_debug_adaptive_chunk(prev) == prev
    assert buf.tobytes() == want.tobytes()


def test_blocking_argument_errors():
    lib = R.load()
    geom = np.zeros((1, 28), np.float32)
    nodes = np.zeros((1, 8), np.float32)
    types = np.zeros(1, np.float32)
    rec = np.zeros((1, 24), np.float32)
    npx = 16 * 9
    rgba = np.full((npx, 4), 3.0, np.float32)
    depth = np.full(npx, 3.0, np.float32)
    err = np.full(npx, 3.0, np.float32)
    count = np.full(npx, 0xCDCDCDCD, np.uint32)
    state = np.frombuffer(bytes([0xCD]) * (npx * 32), R.PASS_STATE_DTYPE).copy()
    aux = np.frombuffer(bytes([0xCD]) * (npx * 16), R.PASS_AUX_DTYPE).copy()
    rounds = C.c_uint32(77)
    cam = R.RtCamera()
    st = R.RtStats()
    texels = np.zeros((2, 2, 3), np.uint8)
    bad_tex = (R.RtTexture * 1)(R.RtTexture(texels.ctypes.data, 2, 0, 3))

    def params(**kw):
        d = dict(width=16, height=9, spp=4, max_bounces=8)
        d.update(kw)
        return R.RtParams(**d)

    def tail():
        return (count.ctypes.data, err.ctypes.data, state.ctypes.data, aux.ctypes.data, C.addressof(rounds), -1,
                C.byref(st))

    def inw(g=geom, n=1, layout=1, nd=nodes, lt=None, nl=0, tex=None, nt=0, c=cam, p=None, batch=2, o=rgba):
        p = params() if p is None else p
        return lib.rt_render_adaptive_inw(R.fptr(g), n, layout, R.fptr(nd), R.fptr(lt), nl, tex, nt,
                                          C.byref(c) if c is not None else None, C.byref(p) if p is not False else None,
                                          batch, 0.1, 2, 0, R.fptr(o.reshape(-1)) if o is not None else None,
                                          R.fptr(depth), *tail())

    def iow(t=types, r=rec, n=1, c=cam, p=None, batch=2, o=rgba):
        p = params() if p is None else p
        return lib.rt_render_adaptive_iow03(R.fptr(t), R.fptr(r), n, C.byref(c) if c is not None else None,
                                            C.byref(p) if p is not False else None, batch, 0.1, 2, 0,
                                            R.fptr(o.reshape(-1)) if o is not None else None, *tail())

    for call in (inw, iow):
        assert call(c=None) == R.RT_E_ARG and call(p=False) == R.RT_E_ARG       # null cam / params
        assert call(n=0) == R.RT_E_ARG and call(o=None) == R.RT_E_ARG
        assert call(batch=0) == R.RT_E_ARG
        for bad in (dict(width=0), dict(height=-1), dict(spp=0), dict(max_bounces=-1)):
            assert call(p=params(**bad)) == R.RT_E_ARG, bad
        assert call(p=params(show_normal=1)) == R.RT_E_UNSUPPORTED              # no fold state in that mode
        assert call(p=params(show_normal=1), batch=0) == R.RT_E_ARG             # argument errors come first
    assert inw(g=None) == R.RT_E_ARG and inw(nd=None) == R.RT_E_ARG
    assert inw(layout=3) == R.RT_E_ARG and inw(layout=0) == R.RT_E_ARG
    assert inw(layout=4, lt=None, nl=1) == R.RT_E_ARG                           # lights counted but not given
    assert inw(layout=4, tex=bad_tex, nt=1) == R.RT_E_ARG                       # a texture without rows
    textured = geom.copy()
    textured[0, 27] = 1.0                                                       # layout 4: TextureIndex 1, none bound
    assert inw(g=textured, layout=4) == R.RT_E_UNSUPPORTED
    assert iow(t=None) == R.RT_E_ARG and iow(r=None) == R.RT_E_ARG
    assert np.all(rgba == 3.0) and np.all(depth == 3.0) and np.all(err == 3.0) and np.all(count == 0xCDCDCDCD)
    assert np.all(state.view(np.uint8) == 0xCD) and np.all(aux.view(np.uint8) == 0xCD)
    assert rounds.value == 77 and st.segments == 0 and st.ms == 0.0
