"""rt_dev_scene_iow03_update and its read-back hooks on a host without a device: the symbols, the
header's contract, and the argument errors, which come back before a device is touched."""
import ctypes as C
import os
import re

import numpy as np

import rt_amd as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rt_dev_scene_iow03_update", "rt_debug_iow_info", "rt_debug_iow_dump")


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def test_symbols_exported_and_mirrored():
    lib = R.load()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in R.SIGNATURES, name
    assert (R.RT_UPDATE_HOST_BUILD, R.RT_UPDATE_DEVICE_BUILD) == (1, 2)
    for fn in (R.update_iow03, R.iow_info, R.iow_dump):
        assert callable(fn)


def test_header_declares_flags_and_prototypes():
    h = _header("rt_hip.h")
    assert re.search(r"^#define\s+RT_UPDATE_HOST_BUILD\s+1\b", h, re.M)
    assert re.search(r"^#define\s+RT_UPDATE_DEVICE_BUILD\s+2\b", h, re.M)
    code = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    assert re.search(r"int\s+rt_dev_scene_iow03_update\s*\(\s*rt_dev_scene\s*\*\s*s\s*,\s*const\s+float\s*\*\s*types\s*,"
                     r"\s*const\s+float\s*\*\s*records\s*,\s*uint32_t\s+n\s*,\s*int\s+flags\s*,\s*double\s+timing_ms\[4\]\s*\)",
                     code)
    assert not re.search(r"rt_debug_iow_", code)  # the hooks live in the debug header
    d = re.sub(r"/\*.*?\*/", "", _header("rt_hip_debug.h"), flags=re.S)
    assert re.search(r"int\s+rt_debug_iow_info\s*\(\s*rt_dev_scene\s*\*\s*s\s*,\s*uint32_t\s+info\[8\]\s*\)", d)
    assert re.search(r"int\s+rt_debug_iow_dump\s*\(\s*rt_dev_scene\s*\*\s*s\s*,\s*uint32_t\s+info\[4\]\s*,\s*float\s*\*\s*wide\s*,"
                     r"\s*float\s*\*\s*obox\s*\)", d)


def test_abi_version_and_options_size_stay():
    assert R.load().rt_abi_version() == R.ABI_VERSION == 5
    assert re.search(r"^#define\s+RT_ABI_VERSION\s+5\b", _header("rt_hip.h"), re.M)
    assert R.default_options().size == C.sizeof(R.RtOptions)


def test_argument_errors_for_a_null_scene():
    """Every argument error with a null scene: RT_E_ARG, nothing read (the record pointers may be
    null too) and nothing written (timing_ms keeps its bytes)."""
    lib = R.load()
    types = np.ones(2, np.float32)
    rec = np.zeros((2, 24), np.float32)
    tm = (C.c_double * 4)(7.0, 7.0, 7.0, 7.0)
    for flags in (0, R.RT_UPDATE_HOST_BUILD, R.RT_UPDATE_DEVICE_BUILD, 3, 4, -1):
        assert lib.rt_dev_scene_iow03_update(None, R.fptr(types), R.fptr(rec), 2, flags, tm) == R.RT_E_ARG
    assert lib.rt_dev_scene_iow03_update(None, None, R.fptr(rec), 2, 0, tm) == R.RT_E_ARG
    assert lib.rt_dev_scene_iow03_update(None, R.fptr(types), None, 2, 0, tm) == R.RT_E_ARG
    assert lib.rt_dev_scene_iow03_update(None, R.fptr(types), R.fptr(rec), 0, 0, tm) == R.RT_E_ARG
    assert lib.rt_dev_scene_iow03_update(None, None, None, 0, 0, None) == R.RT_E_ARG
    assert list(tm) == [7.0] * 4


def test_hooks_refuse_a_null_scene():
    lib = R.load()
    info8 = (C.c_uint32 * 8)(*([9] * 8))
    info4 = (C.c_uint32 * 4)(*([9] * 4))
    assert lib.rt_debug_iow_info(None, info8) == R.RT_E_ARG
    assert lib.rt_debug_iow_info(None, None) == R.RT_E_ARG
    assert lib.rt_debug_iow_dump(None, info4, None, None) == R.RT_E_ARG
    assert lib.rt_debug_iow_dump(None, None, None, None) == R.RT_E_ARG
    assert list(info8) == [9] * 8 and list(info4) == [9] * 4
