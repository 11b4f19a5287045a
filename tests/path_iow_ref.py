"""Builds and calls tests/path_iow_ref.c, the CPU reference of the IOW-03 path-query tests: the
oracle's own launch_rays() per query on a ray stack that holds the incoming RI state, chains, and
out_Pixel's camera rays.  Used by tests/golden/make_path_iow_golden.py (writes the path_iow_*.npz
fixtures), tests/test_path_iow_ref.py (recomputes them) and tests/test_gpu_path_iow.py."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")

# the path_iow_*.npz fixtures, in the order the generator writes them
SETS = ["final", "final_deep", "rot", "ref3", "shells", "one", "state", "cam_final"]
SPP = 8                 # the scatter table of every fixture
CAM_W, CAM_H = 16, 9    # cam_final's frame

RAY_DTYPE = np.dtype([("o", np.float32, 3), ("sample", np.uint32), ("d", np.float32, 3), ("pad", np.uint32),
                      ("ri_in", np.float32, 4)])
OUT_DTYPE = np.dtype([("rgb", np.float32, 3), ("stale", np.uint32), ("segments", np.uint32), ("drops", np.uint32),
                      ("nans", np.uint32), ("status", np.uint32), ("ri_out", np.float32, 4)])


class OrcCamera(C.Structure):
    _fields_ = [("pos", C.c_float * 3), ("dir", C.c_float * 3), ("fov_y_rad", C.c_float),
                ("aperture", C.c_float), ("focus_dist", C.c_float)]


class OrcParams(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("spp", C.c_int), ("max_bounces", C.c_int),
                ("tile_x0", C.c_int), ("tile_y0", C.c_int), ("tile_w", C.c_int), ("tile_h", C.c_int),
                ("show_normal", C.c_int), ("device", C.c_int)]


class OrcStats(C.Structure):
    _fields_ = [("segments", C.c_uint64), ("node_visits", C.c_uint64), ("prim_tests", C.c_uint64),
                ("shadow_queries", C.c_uint64), ("stack_drops", C.c_uint64), ("nan_drops", C.c_uint64),
                ("ms", C.c_double)]


def build(out_dir: str) -> C.CDLL:
    """Compile path_iow_ref.c (with the oracle's sources, its numerics flags) into out_dir and load it."""
    so = os.path.join(str(out_dir), "libpath_iow_ref.so")
    orc = os.path.join(ROOT, "oracle")
    subprocess.run(["gcc", "-O2", "-std=c11", "-D_POSIX_C_SOURCE=200809L", "-fPIC", "-fopenmp", "-ffp-contract=off",
                    "-fno-math-errno", "-shared", "-o", so, os.path.join(HERE, "path_iow_ref.c"),
                    os.path.join(orc, "rt_oracle_host.c"), os.path.join(orc, "rt_oracle_tex.c"), "-lm"], check=True)
    lib = C.CDLL(so)
    lib.path_iow_ref.restype = C.c_int
    lib.path_iow_ref.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_uint32,
                                 C.c_uint32, C.c_void_p, C.c_void_p]
    lib.path_iow_camera.restype = C.c_int
    lib.path_iow_camera.argtypes = [C.POINTER(OrcCamera), C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.orc_render_iow03.restype = C.c_int
    lib.orc_render_iow03.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(OrcCamera), C.POINTER(OrcParams),
                                     C.c_void_p, C.POINTER(OrcStats)]
    return lib


def run(lib, types, records, rays, max_bounces, chain=1, spp=SPP):
    """(out (OUT_DTYPE), counters (3,): segments, drops, nans); asserts that the reference refused no query."""
    types = np.ascontiguousarray(types, np.float32)
    records = np.ascontiguousarray(records, np.float32)
    rays = np.ascontiguousarray(rays, RAY_DTYPE)
    out = np.zeros(rays.shape, OUT_DTYPE)
    ctr = np.zeros(3, np.uint64)
    rc = lib.path_iow_ref(types.ctypes.data, records.ctypes.data, len(types), int(spp), int(max_bounces),
                          rays.ctypes.data, rays.size, int(chain), out.ctypes.data, ctr.ctypes.data)
    assert rc == 0, f"path_iow_ref refused query {rc - 1}" if rc > 0 else "bad arguments"
    return out, ctr


def orc_camera(cam9) -> OrcCamera:
    """cam9: pos3, dir3, fov_y_rad, aperture, focus_dist (float32)."""
    c = OrcCamera()
    v = [float(x) for x in np.asarray(cam9, np.float32)]
    c.pos[:], c.dir[:] = v[0:3], v[3:6]
    c.fov_y_rad, c.aperture, c.focus_dist = v[6], v[7], v[8]
    return c


def camera_rays(lib, cam9, w, h, spp):
    """The frame's camera rays as queries in (y, x, s) order (path_iow_camera), ri_in = 0."""
    rays = np.zeros(w * h * spp, RAY_DTYPE)
    cam = orc_camera(cam9)
    assert lib.path_iow_camera(C.byref(cam), w, h, spp, rays.ctypes.data) == 0
    return rays


def oracle_frame(lib, types, records, cam9, w, h, spp, max_bounces):
    """orc_render_iow03 of the frame: (rgb (w * h, 3) float32, stats dict)."""
    types = np.ascontiguousarray(types, np.float32)
    records = np.ascontiguousarray(records, np.float32)
    cam, st = orc_camera(cam9), OrcStats()
    p = OrcParams(width=w, height=h, spp=spp, max_bounces=max_bounces)
    rgba = np.zeros((h * w, 4), np.float32)
    assert lib.orc_render_iow03(types.ctypes.data, records.ctypes.data, len(types), C.byref(cam), C.byref(p),
                                rgba.ctypes.data, C.byref(st)) == 0
    return rgba[:, :3].copy(), {k: getattr(st, k) for k, _ in st._fields_}


def fold(out, spp):
    """out_Pixel's fold of a frame's answers in (pixel, sample) order (03...glsl:383-417): the samples'
    rgb summed in order in float32, times RN(1 / spp); a pixel stops at its first status = 1 answer
    (the ring schedule's early return), scaled by RN(1 / s).  Returns rgb (pixels, 3) float32."""
    o = out.reshape(-1, spp)
    acc = np.zeros((o.shape[0], 3), np.float32)
    live = np.ones(o.shape[0], bool)
    scale = np.full(o.shape[0], np.float32(1.0) / np.float32(spp), np.float32)
    with np.errstate(all="ignore"):
        for s in range(spp):
            stop = live & (o["status"][:, s] != 0)
            scale[stop] = np.float32(1.0) / np.float32(s)
            live &= ~stop
            acc[live] = acc[live] + o["rgb"][live, s]
        return acc * scale[:, None]


def load_fixture(name: str) -> dict:
    with np.load(os.path.join(GOLDEN, f"path_iow_{name}.npz")) as z:
        d = {k: z[k] for k in z.files}
    d["rays"] = d["rays"].view(RAY_DTYPE).reshape(-1)
    d["out"] = d["out"].view(OUT_DTYPE).reshape(-1)
    d["chain"], d["max_bounces"] = int(d["chain"]), int(d["max_bounces"])
    return d


def same(a, b) -> bool:
    """Bit for bit."""
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def canon(out):
    """A copy of answers (OUT_DTYPE) with every NaN in rgb replaced by one NaN.  A query with a NaN
    direction misses and returns its background colour, NaN arithmetic; IEEE 754 leaves the sign and
    payload of such a NaN to the implementation, and the CPU's and the GPU's differ.  Every other
    field, and every rgb that is a number, keeps its bits."""
    out = out.copy()
    rgb = out["rgb"]
    rgb[np.isnan(rgb)] = np.float32(np.nan)
    return out
