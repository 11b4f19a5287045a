"""Builds and calls tests/path_ref.c, the CPU reference of the path-query tests: the oracle's sample
loop restarted from a given ray, the camera rays inw_sample forms, and inw_sample itself per sample.
Used by tests/golden/make_path_golden.py (writes the paths_*.npz fixtures), tests/test_path_ref.py
(recomputes them) and tests/test_gpu_paths.py (loads them)."""
import ctypes as C
import os
import subprocess
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")

# the paths_*.npz fixtures, in the order the generator writes them
SCENES = ["glass600", "glass600_b", "pile100", "mixed300", "one", "cornell", "refset_tex", "cam_random600",
          "cam_cornell"]
CAM = ["cam_random600", "cam_cornell"]  # every ray a camera ray of a CAM_W x CAM_H frame, order (y, x, s)
CAM_W, CAM_H = 16, 9
SPP = 16

RAY_DTYPE = np.dtype([("o", np.float32, 3), ("sample", np.uint32), ("d", np.float32, 3), ("pad", np.uint32)])
OUT_DTYPE = np.dtype([("rgb", np.float32, 3), ("depth", np.float32), ("segments", np.uint32), ("drops", np.uint32),
                      ("nans", np.uint32), ("status", np.uint32)])


class _Tex(C.Structure):  # orc_texture
    _fields_ = [("texels", C.c_void_p), ("width", C.c_int), ("height", C.c_int), ("channels", C.c_int)]


class Camera(C.Structure):  # orc_camera == rt_camera
    _fields_ = [("pos", C.c_float * 3), ("dir", C.c_float * 3), ("fov_y_rad", C.c_float), ("aperture", C.c_float),
                ("focus_dist", C.c_float)]


def camera_of(v) -> Camera:
    """Camera from 9 floats (pos, dir, fov_y_rad, aperture, focus_dist) or an rt_camera."""
    if not isinstance(v, np.ndarray):
        v = np.array(list(v.pos) + list(v.dir) + [v.fov_y_rad, v.aperture, v.focus_dist], np.float32)
    c = Camera()
    c.pos[:], c.dir[:] = [float(x) for x in v[0:3]], [float(x) for x in v[3:6]]
    c.fov_y_rad, c.aperture, c.focus_dist = float(v[6]), float(v[7]), float(v[8])
    return c


def camera_invert(v) -> int:
    """The child order a frame of this camera (9 floats) renders with: dot(dir, (1, 1, 1)) > 0 in float32."""
    d = np.asarray(v, np.float32)[3:6]
    return int(np.float32(np.float32(d[0] + d[1]) + d[2]) > 0)


def build(out_dir: str) -> C.CDLL:
    """Compile path_ref.c (with the oracle's sources, its numerics flags) into out_dir and load it."""
    so = os.path.join(str(out_dir), "libpath_ref.so")
    orc = os.path.join(ROOT, "oracle")
    subprocess.run(["gcc", "-O2", "-std=c11", "-D_POSIX_C_SOURCE=200809L", "-fPIC", "-fopenmp", "-ffp-contract=off",
                    "-fno-math-errno", "-shared", "-o", so, os.path.join(HERE, "path_ref.c"),
                    os.path.join(orc, "rt_oracle_host.c"), os.path.join(orc, "rt_oracle_tex.c"), "-lm"], check=True)
    lib = C.CDLL(so)
    scene = [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    lib.path_ref.restype = C.c_int
    lib.path_ref.argtypes = scene + [C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p]
    lib.path_camera_rays.restype = C.c_int
    lib.path_camera_rays.argtypes = [C.POINTER(Camera), C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.path_inw_samples.restype = C.c_int
    lib.path_inw_samples.argtypes = scene + [C.POINTER(Camera), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                             C.c_void_p]
    return lib


def _scene_args(fx):
    geom = np.ascontiguousarray(fx.geom, np.float32)
    nodes = np.ascontiguousarray(fx.nodes, np.float32)
    lights = np.ascontiguousarray(fx.lights, np.float32) if fx.n_lights else None
    keep = [np.ascontiguousarray(t, np.uint8) for t in (fx.textures or [])]
    arr = (_Tex * max(1, len(keep)))()
    for i, t in enumerate(keep):
        arr[i] = _Tex(t.ctypes.data, t.shape[1], t.shape[0], t.shape[2])
    args = [geom.ctypes.data, geom.shape[0], int(fx.layout), nodes.ctypes.data,
            lights.ctypes.data if lights is not None else None, int(fx.n_lights), C.addressof(arr), len(keep)]
    return args, (geom, nodes, lights, keep, arr)


def run(lib, fx, rays, invert):
    """(out (OUT_DTYPE), counters uint64[6]) of the restated loop for `rays` on the fixture's scene."""
    rays = np.ascontiguousarray(rays, RAY_DTYPE)
    out = np.zeros(rays.shape, OUT_DTYPE)
    ctr = np.zeros(6, np.uint64)
    args, keep = _scene_args(fx)
    rc = lib.path_ref(*args, int(fx.spp), int(fx.max_bounces), rays.ctypes.data, rays.size, int(invert),
                      out.ctypes.data, ctr.ctypes.data)
    assert rc == 0, rc
    del keep
    return out, ctr


def camera_rays(lib, cam, w, h, spp):
    """The single-focus camera rays of a w x h frame, rays[(y * w + x) * spp + s]."""
    rays = np.zeros(w * h * spp, RAY_DTYPE)
    c = camera_of(cam)
    assert lib.path_camera_rays(C.byref(c), w, h, spp, rays.ctypes.data) == 0
    return rays


def inw_samples(lib, fx, cam, w, h):
    """inw_sample for every (y, x, s): (out (OUT_DTYPE), counters uint64[6])."""
    out = np.zeros(w * h * fx.spp, OUT_DTYPE)
    ctr = np.zeros(6, np.uint64)
    args, keep = _scene_args(fx)
    c = camera_of(cam)
    rc = lib.path_inw_samples(*args, C.byref(c), w, h, int(fx.spp), int(fx.max_bounces), out.ctypes.data,
                              ctr.ctypes.data)
    assert rc == 0, rc
    del keep
    return out, ctr


def fold(out, spp):
    """End() over path outputs ordered (pixel, s): float32, the first sample's sqrt(colour) assigned,
    the others added in order, times 1 / spp; the depth of sample spp / 2.  -> (rgb (P, 3), depth (P,))."""
    rgb = out["rgb"].reshape(-1, spp, 3)
    acc = np.sqrt(rgb[:, 0, :]).astype(np.float32)
    for s in range(1, spp):
        acc = (acc + np.sqrt(rgb[:, s, :]).astype(np.float32)).astype(np.float32)
    inv = np.float32(1.0) / np.float32(spp)
    return (acc * inv).astype(np.float32), out["depth"].reshape(-1, spp)[:, spp // 2].copy()


def load_fixture(name: str) -> SimpleNamespace:
    """A fixture as a packed scene (what rt_amd.paths takes: geom, nodes, layout, lights, textures,
    params.spp) with its rays, max_bounces and, per child order, the outputs and six counters."""
    with np.load(os.path.join(GOLDEN, f"paths_{name}.npz")) as z:
        d = {k: z[k] for k in z.files}
    fx = SimpleNamespace(name=name, geom=d["geom"], aabbs=d["aabbs"], nodes=d["nodes"], layout=int(d["layout"]),
                         lights=d["lights"], n_lights=len(d["lights"]), spp=int(d["spp"]),
                         max_bounces=int(d["max_bounces"]), rays=d["rays"].view(RAY_DTYPE).reshape(-1),
                         out=(d["out0"].view(OUT_DTYPE).reshape(-1), d["out1"].view(OUT_DTYPE).reshape(-1)),
                         ctr=(d["ctr0"], d["ctr1"]), camera=d["camera"] if "camera" in d else None)
    fx.n = fx.geom.shape[0]
    fx.textures = [d[f"tex{i}"] for i in range(int(d["n_tex"]))] or None
    fx.params = SimpleNamespace(spp=fx.spp)
    return fx


def same(a, b) -> bool:
    """Bit for bit."""
    return a.shape == b.shape and a.tobytes() == b.tobytes()
