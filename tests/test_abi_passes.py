"""The progressive-pass entry points of the C ABI without a device: the library exports them and the
Python mirror declares them, rt_pass_state has its stated layout, the header holds the contract, and
every argument error that needs no scene comes back before any device is touched, with the buffers
untouched.  (The errors that need a scene -- another spp, s0 >= spp -- are in tests/test_gpu_passes.py.)"""
import ctypes as C
import os
import re

import numpy as np

import rt_amd as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rt_render_pass_async", "rt_render_passes_inw", "rt_render_passes_iow03", "rt_debug_pass_kernel",
         "rt_debug_pass_max_blocks")


def test_exported_and_mirrored():
    lib = R.load()
    for name in NAMES:
        assert name in R.SIGNATURES and hasattr(lib, name), name
    for name in ("render_passes", "pass_kernel_info", "PASS_STATE_DTYPE", "PASS_KERNELS"):
        assert hasattr(R, name), name
    assert R.ABI_VERSION == 5 and lib.rt_abi_version() == 5  # additive: the version stays
    assert C.sizeof(R.RtOptions) == R.default_options().size    # rt_options is unchanged


def test_state_layout():
    d = R.PASS_STATE_DTYPE
    assert d.itemsize == 32
    assert [d.fields[k][1] for k in ("acc", "depth", "ri")] == [0, 12, 16]
    assert d["acc"].shape == (3,) and d["ri"].shape == (4,) and d["depth"] == np.float32
    assert d["acc"].base == np.float32 and d["ri"].base == np.float32


def test_header_declares_the_passes():
    src = open(os.path.join(ROOT, "include", "rt_hip.h")).read()
    assert "typedef struct rt_pass_state { float acc[3]; float depth; float ri[4]; } rt_pass_state;" in src
    assert re.search(r"#define\s+RT_ABI_VERSION\s+5\b", src)
    assert src.index("rt_pixels_iow03(") < src.index("rt_render_pass_async(") < src.index("rt_render_passes_inw(") < \
        src.index("rt_render_passes_iow03(") < src.index("rt_tile_deal(")
    flat = " ".join(src.split())
    for phrase in ("uint32_t s0, uint32_t ns, rt_pass_state *d_state", "acc * RN(1 / k)", "bit for bit",
                   "s0 >= p->spp", "ns == 0 returns RT_OK", "the pass is clipped", "early-return marker",
                   "With s0 == 0 the incoming state is not read", "Pixels outside the rectangle keep their state",
                   "graph-capturable", "later passes allocate nothing", "MULTIFOCUS"):
        assert phrase in flat, phrase
    dbg = open(os.path.join(ROOT, "include", "rt_hip_debug.h")).read()
    assert "int rt_debug_pass_kernel(int which, int info[4]);" in dbg
    assert "int rt_debug_pass_max_blocks(int blocks);" in dbg


def test_async_argument_errors():
    """A null scene is an error whatever else is passed, before any pointer is read or written."""
    lib = R.load()
    cam, p = R.RtCamera(), R.RtParams(width=16, height=9, spp=4, max_bounces=8)
    buf = np.full(64, 7.0, np.float32)
    want = buf.copy()
    b = buf.ctypes.data
    for s0, ns in ((0, 4), (0, 0), (2, 1), (4, 1), (0, 0xFFFFFFFF)):
        assert lib.rt_render_pass_async(None, C.byref(cam), C.byref(p), s0, ns, b, b, b, b, None) == R.RT_E_ARG
    assert lib.rt_render_pass_async(None, None, None, 0, 1, None, None, None, None, None) == R.RT_E_ARG
    assert lib.rt_debug_pass_kernel(0, None) == R.RT_E_ARG
    info = (C.c_int * 4)()
    assert lib.rt_debug_pass_kernel(4, info) == R.RT_E_ARG and lib.rt_debug_pass_kernel(-1, info) == R.RT_E_ARG
    prev = lib.rt_debug_pass_max_blocks(3)
    assert lib.rt_debug_pass_max_blocks(-5) == 3 and lib.rt_debug_pass_max_blocks(prev) == 0  # negative: no cap
    assert lib.rt_debug_pass_max_blocks(prev) == prev
    assert buf.tobytes() == want.tobytes()


def test_blocking_argument_errors():
    lib = R.load()
    geom = np.zeros((1, 28), np.float32)
    nodes = np.zeros((1, 8), np.float32)
    types = np.zeros(1, np.float32)
    rec = np.zeros((1, 24), np.float32)
    npx = 16 * 9
    rgba = np.full((2, npx, 4), 3.0, np.float32)
    depth = np.full((2, npx), 3.0, np.float32)
    state = np.frombuffer(bytes([0xCD]) * (npx * 32), R.PASS_STATE_DTYPE).copy()
    cam = R.RtCamera()
    st = R.RtStats()
    texels = np.zeros((2, 2, 3), np.uint8)
    bad_tex = (R.RtTexture * 1)(R.RtTexture(texels.ctypes.data, 2, 0, 3))
    good = (2, 4)

    def params(**kw):
        d = dict(width=16, height=9, spp=4, max_bounces=8)
        d.update(kw)
        return R.RtParams(**d)

    def cuts_of(cuts):
        if cuts is None:
            return None, 2
        a = (C.c_uint32 * max(1, len(cuts)))(*cuts)
        return a, len(cuts)

    def inw(g=geom, n=1, layout=1, nd=nodes, lt=None, nl=0, tex=None, nt=0, c=cam, p=None, cuts=good, o=rgba):
        p = params() if p is None else p
        a, nc = cuts_of(cuts)
        return lib.rt_render_passes_inw(R.fptr(g), n, layout, R.fptr(nd), R.fptr(lt), nl, tex, nt,
                                        C.byref(c) if c is not None else None, C.byref(p) if p is not False else None,
                                        a, nc, R.fptr(o.reshape(-1)) if o is not None else None, R.fptr(depth.reshape(-1)),
                                        state.ctypes.data, -1, C.byref(st))

    def iow(t=types, r=rec, n=1, c=cam, p=None, cuts=good, o=rgba):
        p = params() if p is None else p
        a, nc = cuts_of(cuts)
        return lib.rt_render_passes_iow03(R.fptr(t), R.fptr(r), n, C.byref(c) if c is not None else None,
                                          C.byref(p) if p is not False else None, a, nc,
                                          R.fptr(o.reshape(-1)) if o is not None else None, state.ctypes.data, -1,
                                          C.byref(st))

    for call in (inw, iow):
        assert call(c=None) == R.RT_E_ARG and call(p=False) == R.RT_E_ARG       # null cam / params
        assert call(n=0) == R.RT_E_ARG and call(o=None) == R.RT_E_ARG
        for bad in (dict(width=0), dict(height=-1), dict(spp=0), dict(max_bounces=-1)):
            assert call(p=params(**bad)) == R.RT_E_ARG, bad
        # cuts: null, none, starting at 0, not increasing, decreasing, past spp
        for bad in (None, (), (0, 4), (2, 2), (3, 2), (2, 5), (5,)):
            assert call(cuts=bad) == R.RT_E_ARG, bad
        assert call(p=params(show_normal=1)) == R.RT_E_UNSUPPORTED              # no fold state in that mode
        assert call(p=params(show_normal=1), cuts=(0, 4)) == R.RT_E_ARG         # argument errors come first
    assert inw(g=None) == R.RT_E_ARG and inw(nd=None) == R.RT_E_ARG
    assert inw(layout=3) == R.RT_E_ARG and inw(layout=0) == R.RT_E_ARG
    assert inw(layout=4, lt=None, nl=1) == R.RT_E_ARG                           # lights counted but not given
    assert inw(layout=4, tex=bad_tex, nt=1) == R.RT_E_ARG                       # a texture without rows
    textured = geom.copy()
    textured[0, 27] = 1.0                                                       # layout 4: TextureIndex 1, none bound
    assert inw(g=textured, layout=4) == R.RT_E_UNSUPPORTED
    assert iow(t=None) == R.RT_E_ARG and iow(r=None) == R.RT_E_ARG
    assert np.all(rgba == 3.0) and np.all(depth == 3.0) and np.all(state.view(np.uint8) == 0xCD)
    assert st.segments == 0 and st.ms == 0.0
