"""The C ABI surface of librt_hip.so: it loads on a CPU-only host, exports every function
include/*.h declares, and validates arguments before touching a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rt_amd as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(headers=("rt_hip.h", "rt_hip_debug.h", "rt_scene.h")):
    names = set()
    for h in headers:
        src = open(os.path.join(ROOT, "include", h)).read()
        src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
        for m in re.finditer(r"^\s*(?:int|void|size_t|rt_dev_scene\s*\*|rt_group\s*\*)\s*\*?\s*(rt_\w+)\s*\(", src, re.M):
            names.add(m.group(1))
    return names


def test_library_exports_every_declared_symbol():
    lib = R.load()
    declared = _declared()
    assert len(declared) >= 16
    for name in declared:
        assert hasattr(lib, name), name
    assert declared == set(R.SIGNATURES), declared ^ set(R.SIGNATURES)


def test_render_header_declares_no_debug_symbol():
    """The diagnostics and test hooks live in rt_hip_debug.h; rt_hip.h alone is the render ABI."""
    assert not [n for n in _declared(("rt_hip.h",)) if n.startswith("rt_debug_")]
    assert [n for n in _declared(("rt_hip_debug.h",)) if n.startswith("rt_debug_")]


def test_abi_version():
    assert R.load().rt_abi_version() == R.ABI_VERSION == 5


def test_options_roundtrip_and_validation():
    """rt_options: the defaults are the measured-best settings, set / get round-trip, and
    out-of-range values are rejected (the options stay as they were)."""
    lib = R.load()
    d = R.default_options()
    assert d.size == C.sizeof(R.RtOptions)
    assert (d.inw_wide_walk, d.inw_order, d.inw_beams, d.inw_ring_pm, d.inw_ring_sm) == (1, 0, 1, 0, 0)
    assert (d.iow_spec, d.spec_rounds, d.spec_tail_rounds, d.spec_tail_budget) == (1, 24, 60, 3072)
    with R.options(inw_order=2, spec_iters=3) as o:
        g = R.get_options()
        assert g.inw_order == 2 and g.spec_iters == 3 and g.as_dict() == o.as_dict()
    assert R.get_options().as_dict() == d.as_dict()
    for field, bad in (("inw_ring_pm", 100), ("inw_ring_sm", 32), ("inw_order", 3), ("rounds_seq", 15),
                       ("iow_leaf_batch", 0), ("spec_alt_cap", 1), ("spec_max_gb", 0.0)):
        o = R.default_options()
        setattr(o, field, bad)
        assert lib.rt_options_set(C.byref(o)) == R.RT_E_ARG, field
    o = R.default_options()
    o.size = 8
    assert lib.rt_options_set(C.byref(o)) == R.RT_E_ARG
    assert lib.rt_options_set(None) == R.RT_E_ARG
    assert R.get_options().as_dict() == d.as_dict()
    with pytest.raises(KeyError):
        with R.options(no_such_option=1):
            pass
    assert lib.rt_dev_scene_set_options(None, C.byref(d)) == R.RT_E_ARG
    assert lib.rt_debug_path(None, None) == R.RT_E_ARG


def test_render_path_reads_no_environment():
    """What the library runs is set through rt_options only: the product sources read no
    environment variable outside the diagnostic builds (#ifdef RT_DIAG)."""
    csrc = os.path.join(ROOT, "raytracing-tests_amd", "csrc")
    for fn in sorted(os.listdir(csrc)):
        depth, in_diag = 0, []
        for i, line in enumerate(open(os.path.join(csrc, fn)), 1):
            t = line.strip()
            if t.startswith("#if"):
                in_diag.append("RT_DIAG" in t)
            elif t.startswith("#endif") and in_diag:
                in_diag.pop()
            if "getenv" in t and not t.startswith("//"):
                assert any(in_diag), f"{fn}:{i}: getenv outside #ifdef RT_DIAG"


def test_argument_validation_without_device():
    lib = R.load()
    st = R.RtStats()
    cam = R.RtCamera()
    p = R.RtParams(0, 0, 1, 1, 0, 0, 0, 0, 0, -1)
    buf = np.zeros(16, np.float32)
    assert lib.rt_render_iow01(None, None, None, None, None) == R.RT_E_ARG
    assert lib.rt_render_iow03(R.fptr(buf), R.fptr(buf), 1, C.byref(cam), C.byref(p), R.fptr(buf), C.byref(st)) == R.RT_E_ARG
    p.width = p.height = 4
    assert lib.rt_render_inw(R.fptr(buf), 1, 3, R.fptr(buf), None, 0, C.byref(cam), C.byref(p), R.fptr(buf), None,
                             C.byref(st)) == R.RT_E_ARG  # bad layout
    assert lib.rt_lbvh_build(None, 0, None) == R.RT_E_ARG
    assert lib.rt_sample_tables(0, None, None, None) == R.RT_E_ARG
    assert lib.rt_scene_preset(999, 0, 0, None, 0, None, None) == R.RT_E_ARG
    assert lib.rt_render_tiles_async(None, None, None, None, 0, 16, None, None, None, None) == R.RT_E_ARG
    assert lib.rt_dev_scene_inw_update(None, R.fptr(buf), 1, None, None, None, 0, None) == R.RT_E_ARG


def test_textured_records_rejected_before_device():
    sc = R.make_scene(R.PRESET_INW04_REFSET, spp=1)
    sc.geom[1, 27] = 2.0
    lib = R.load()
    rgba = np.zeros((100, 100, 4), np.float32)
    rc = lib.rt_render_inw(R.fptr(sc.geom), sc.n, 4, R.fptr(sc.nodes), R.fptr(sc.lights), sc.n_lights,
                           C.byref(sc.camera), C.byref(sc.params), R.fptr(rgba), None, None)
    assert rc == R.RT_E_UNSUPPORTED


def test_no_silent_cpu_fallback():
    """Without a GPU the product path reports an error; it never renders on the CPU."""
    from conftest import gpu_available
    if gpu_available():
        pytest.skip("GPU present")
    cam, sph, p = R.iow01_defaults(8, 8)
    with pytest.raises(RuntimeError):
        R.render_iow01(cam, sph, p)


def test_product_does_not_reference_oracle():
    """The shipped library and the product Python package never name the oracle."""
    with open(R.LIB_PATH, "rb") as f:
        blob = f.read()
    assert b"orc_" not in blob and b"librt_oracle" not in blob
    pkg = os.path.join(ROOT, "raytracing-tests_amd", "rt_amd")
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            assert "oracle" not in open(os.path.join(pkg, fn)).read().replace("no CPU fallback", ""), fn
