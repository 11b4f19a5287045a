"""rt_dev_scene_inw_update_device, rt_inw_swept_boxes_async and the record dumps on a host without a
device: the symbols, the header's contract, and the argument errors, which come back before a device is
touched."""
import ctypes as C
import os
import re

import rt_amd as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rt_dev_scene_inw_update_device", "rt_inw_swept_boxes_async", "rt_debug_update_kernel")
PTR = 0x1000  # a non-null "device pointer": argument errors read nothing


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def test_symbols_exported_and_mirrored():
    lib = R.load()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in R.SIGNATURES, name
    assert (R.RT_UPDATE_BINS, R.RT_UPDATE_NO_BINS) == (4, 8)
    assert (R.RT_WALK_HOT, R.RT_WALK_COLD, R.RT_WALK_SPH) == (9, 10, 11)
    for fn in (R.update_inw_device, R.inw_swept_boxes, R.update_kernel_info):
        assert callable(fn)


def test_header_declares_flags_and_prototypes():
    h = _header("rt_hip.h")
    assert re.search(r"^#define\s+RT_UPDATE_BINS\s+4\b", h, re.M)
    assert re.search(r"^#define\s+RT_UPDATE_NO_BINS\s+8\b", h, re.M)
    code = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    assert re.search(r"int\s+rt_dev_scene_inw_update_device\s*\(\s*rt_dev_scene\s*\*\s*s\s*,\s*const\s+float\s*\*\s*d_geom\s*,"
                     r"\s*uint32_t\s+n\s*,\s*const\s+float\s*\*\s*d_aabbs\s*,\s*const\s+float\s*\*\s*d_lights\s*,"
                     r"\s*uint32_t\s+n_lights\s*,\s*int\s+flags\s*,\s*void\s*\*\s*stream\s*,\s*double\s+timing_ms\[4\]\s*\)",
                     code)
    assert re.search(r"int\s+rt_inw_swept_boxes_async\s*\(\s*const\s+float\s*\*\s*d_geom\s*,\s*uint32_t\s+n\s*,"
                     r"\s*float\s*\*\s*d_aabbs_out\s*,\s*void\s*\*\s*stream\s*\)", code)
    at = h.index("int rt_inw_swept_boxes_async")  # its comment says how its boxes differ from the packer's
    assert "rt_pack_inw" in h[at - 1200:at]
    d = _header("rt_hip_debug.h")
    for name, v in (("RT_WALK_HOT", 9), ("RT_WALK_COLD", 10), ("RT_WALK_SPH", 11)):
        assert re.search(rf"^#define\s+{name}\s+{v}\b", d, re.M), name


def test_abi_version_and_options_size_stay():
    assert R.load().rt_abi_version() == R.ABI_VERSION == 5
    assert re.search(r"^#define\s+RT_ABI_VERSION\s+5\b", _header("rt_hip.h"), re.M)
    assert R.default_options().size == C.sizeof(R.RtOptions)


def test_argument_errors_for_a_null_scene():
    """Every argument error with a null scene: RT_E_ARG, nothing read and nothing written (timing_ms keeps
    its bytes)."""
    lib = R.load()
    tm = (C.c_double * 4)(7.0, 7.0, 7.0, 7.0)
    up = lib.rt_dev_scene_inw_update_device
    for flags in (0, R.RT_UPDATE_BINS, R.RT_UPDATE_NO_BINS, 12, 16, 1, 2, -1):
        assert up(None, PTR, 2, PTR, None, 0, flags, None, tm) == R.RT_E_ARG, flags
    assert up(None, None, 2, PTR, None, 0, 0, None, tm) == R.RT_E_ARG
    assert up(None, PTR, 2, None, None, 0, 0, None, tm) == R.RT_E_ARG
    assert up(None, PTR, 0, PTR, None, 0, 0, None, tm) == R.RT_E_ARG
    assert up(None, PTR, 2, PTR, None, 3, 0, None, tm) == R.RT_E_ARG
    assert up(None, None, 0, None, None, 0, 0, None, None) == R.RT_E_ARG
    assert list(tm) == [7.0] * 4


def test_swept_boxes_refuses_null_pointers():
    lib = R.load()
    assert lib.rt_inw_swept_boxes_async(None, 4, PTR, None) == R.RT_E_ARG
    assert lib.rt_inw_swept_boxes_async(PTR, 4, None, None) == R.RT_E_ARG
    assert lib.rt_inw_swept_boxes_async(None, 0, None, None) == R.RT_E_ARG


def test_record_dumps_refuse_a_null_scene():
    lib = R.load()
    info = (C.c_uint64 * 8)(*([9] * 8))
    for what in (R.RT_WALK_HOT, R.RT_WALK_COLD, R.RT_WALK_SPH):
        assert lib.rt_debug_walk_dump(None, what, None, 0, info) == R.RT_E_ARG
        assert lib.rt_debug_walk_dump(None, what, None, 0, None) == R.RT_E_ARG
    assert list(info) == [9] * 8
    assert lib.rt_debug_update_kernel(0, None) == R.RT_E_ARG
    assert lib.rt_debug_update_kernel(4, (C.c_int * 4)()) == R.RT_E_ARG
