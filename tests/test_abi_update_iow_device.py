"""rt_dev_scene_iow03_update_device and its debug surface on a host without a device: the symbols, the
header's contract, and the argument errors, which come back before a device is touched."""
import ctypes as C
import os
import re

import rt_amd as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rt_dev_scene_iow03_update_device", "rt_debug_iow_prepare_host", "rt_debug_iow_records",
       "rt_debug_update_iow_kernel")
PTR = 0x1000  # a non-null "device pointer": argument errors read nothing


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def test_symbols_exported_and_mirrored():
    lib = R.load()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in R.SIGNATURES, name
    assert (R.RT_UPDATE_HOST_BUILD, R.RT_UPDATE_DEVICE_BUILD) == (1, 2)
    for fn in (R.update_iow03_device, R.iow_prepare_host, R.iow_records, R.update_iow_kernel_info):
        assert callable(fn)
    assert len(R.UPDATE_IOW_KERNELS) == 4


def test_header_declares_the_prototypes_and_the_flag_rule():
    h = _header("rt_hip.h")
    assert re.search(r"^#define\s+RT_UPDATE_HOST_BUILD\s+1\b", h, re.M)
    assert re.search(r"^#define\s+RT_UPDATE_DEVICE_BUILD\s+2\b", h, re.M)
    code = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    assert re.search(r"int\s+rt_dev_scene_iow03_update_device\s*\(\s*rt_dev_scene\s*\*\s*s\s*,\s*const\s+float\s*\*\s*d_types\s*,"
                     r"\s*const\s+float\s*\*\s*d_records\s*,\s*uint32_t\s+n\s*,\s*int\s+flags\s*,\s*void\s*\*\s*stream\s*,"
                     r"\s*double\s+timing_ms\[4\]\s*\)", code)
    at = h.index("int rt_dev_scene_iow03_update_device")
    text = " ".join(h[at - 4000:at].replace("*", " ").split())  # its comment, the flags = 0 rule and its reason
    for words in ("from 1024 objects", "486 objects", "2.1%", "copied back once", "RT_UPDATE_DEVICE_BUILD: no record byte",
                  "16-byte aligned", "4-byte alignment", "before a device is touched"):
        assert words in text, words
    d = re.sub(r"/\*.*?\*/", "", _header("rt_hip_debug.h"), flags=re.S)
    assert re.search(r"int\s+rt_debug_iow_prepare_host\s*\(\s*const\s+float\s*\*\s*types\s*,\s*const\s+float\s*\*\s*records\s*,"
                     r"\s*uint32_t\s+n\s*,\s*float\s*\*\s*hot\s*,\s*float\s*\*\s*cold\s*,\s*float\s+priors\[10\]\s*\)", d)
    assert re.search(r"int\s+rt_debug_iow_records\s*\(\s*rt_dev_scene\s*\*\s*s\s*,\s*float\s*\*\s*hot\s*,\s*float\s*\*\s*cold\s*,"
                     r"\s*float\s+priors\[10\]\s*\)", d)
    assert re.search(r"int\s+rt_debug_update_iow_kernel\s*\(\s*int\s+which\s*,\s*int\s+info\[4\]\s*\)", d)


def test_abi_version_and_options_size_stay():
    assert R.load().rt_abi_version() == R.ABI_VERSION == 5
    assert re.search(r"^#define\s+RT_ABI_VERSION\s+5\b", _header("rt_hip.h"), re.M)
    assert R.default_options().size == C.sizeof(R.RtOptions)


def test_argument_errors_for_a_null_scene():
    """Every argument error with a null scene: RT_E_ARG, nothing read and nothing written (timing_ms keeps
    its bytes)."""
    lib = R.load()
    tm = (C.c_double * 4)(7.0, 7.0, 7.0, 7.0)
    up = lib.rt_dev_scene_iow03_update_device
    for flags in (0, R.RT_UPDATE_HOST_BUILD, R.RT_UPDATE_DEVICE_BUILD, 3, 4, 8, -1):
        assert up(None, PTR, PTR, 2, flags, None, tm) == R.RT_E_ARG, flags
    assert up(None, None, PTR, 2, 0, None, tm) == R.RT_E_ARG
    assert up(None, PTR, None, 2, 0, None, tm) == R.RT_E_ARG
    assert up(None, PTR, PTR, 0, 0, None, tm) == R.RT_E_ARG
    assert up(None, None, None, 0, 0, None, None) == R.RT_E_ARG
    assert list(tm) == [7.0] * 4


def test_debug_dumps_refuse_a_null_scene():
    lib = R.load()
    pri = (C.c_float * 10)(*([9.0] * 10))
    assert lib.rt_debug_iow_records(None, None, None, pri) == R.RT_E_ARG
    assert lib.rt_debug_iow_records(None, None, None, None) == R.RT_E_ARG
    assert list(pri) == [9.0] * 10
    assert lib.rt_debug_update_iow_kernel(0, None) == R.RT_E_ARG
    assert lib.rt_debug_update_iow_kernel(4, (C.c_int * 4)()) == R.RT_E_ARG
    assert lib.rt_debug_update_iow_kernel(-1, (C.c_int * 4)()) == R.RT_E_ARG
