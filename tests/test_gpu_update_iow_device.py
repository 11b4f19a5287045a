"""rt_dev_scene_iow03_update_device: the next edit of an IOW-03 device scene from types and records that
live on the device.  The hot and cold records and the RI priors its kernels make must be the host
packer's byte for byte (rt_debug_iow_prepare_host, itself tied to numpy by tests/test_iow_prepare_ref.py);
after the update the scene must behave as a fresh scene of the same records: frames, counters, queries and
passes byte-equal, the device-built structures conservative when checked directly.

Scenes as in tests/test_gpu_update_iow.py: the records of PRESET_IOW03_FINAL with the benchmark's seed (config
C2, 486 objects), sliced to their first k objects or tiled with offsets; state 1 moves every object of
state 0."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

import rt_amd as R
import iow_prepare_ref as P
from oracle import oracle as O
from walk_struct_ref import check_iow_cull

pytestmark = pytest.mark.gpu

HOST, DEVICE = R.RT_UPDATE_HOST_BUILD, R.RT_UPDATE_DEVICE_BUILD
W, H, SPP, BOUNCES = 48, 32, 6, 8
N_BASE = 486
DEVICE_BUILD_MIN = 1024  # flags = 0: the device build from here on (rt_dev_scene_iow03_update's rule)
_cache = {}


def base():
    if "base" not in _cache:
        _cache["base"] = R.make_scene(R.PRESET_IOW03_FINAL, 20250131, 0, width=W, height=H, spp=SPP, max_bounces=BOUNCES)
        assert _cache["base"].n == N_BASE
    return _cache["base"]


def small_params(sc):
    """16 x 16 pixels, 2 spp: the frames of the largest scenes."""
    p = R.RtParams.from_buffer_copy(bytes(sc.params))
    p.width, p.height, p.spp = 16, 16, 2
    return p


def scene_of(n, state=0):
    """n objects from the base records (the first n, or whole copies tiled 24 apart in x and z), every
    object moved in state 1."""
    key = ("scene", n, state)
    if key in _cache:
        return _cache[key]
    b = base()
    idx = np.arange(n) % N_BASE
    copy = np.arange(n) // N_BASE
    rec = b.records[idx].copy()
    types = b.types[idx].copy()
    rec[:, 0] += (24.0 * (copy % 6)).astype(np.float32)
    rec[:, 2] -= (24.0 * (copy // 6)).astype(np.float32)
    if state:
        i = np.arange(n)
        for k in range(3):
            rec[:, k] += (0.05 * ((i + k) % 3 - 1)).astype(np.float32)
    sc = dataclasses.replace(b, n=n, types=np.ascontiguousarray(types), records=np.ascontiguousarray(rec), desc=None)
    if n > 2000:
        sc = dataclasses.replace(sc, params=small_params(sc))
    _cache[key] = sc
    return sc


def with_records(types, rec):
    """A scene of the base's camera and params with these types and records."""
    types = np.ascontiguousarray(types, np.float32)
    rec = np.ascontiguousarray(rec, np.float32).reshape(-1, 24)
    sc = dataclasses.replace(base(), n=len(types), types=types, records=rec, desc=None)
    return dataclasses.replace(sc, params=small_params(sc)) if len(types) > 2000 else sc


def frame(s, sc, stream=None, expect=R.RT_OK):
    """One frame of device scene s with sc's camera and params: (rgba bytes, the six counters)."""
    p = sc.params
    dev = torch.device("cuda")
    st = stream or torch.cuda.current_stream()
    with torch.cuda.stream(st):
        img = torch.zeros((p.height, p.width, 4), dtype=torch.float32, device=dev)
        ctr = torch.zeros(6, dtype=torch.int64, device=dev)
    st.synchronize()
    rc = R.load().rt_render_image_async(s, C.byref(sc.camera), C.byref(p), img.data_ptr(), None, ctr.data_ptr(),
                                        st.cuda_stream)
    assert rc == expect
    st.synchronize()
    return img.cpu().numpy().tobytes(), [int(x) for x in ctr.cpu().numpy()]


def scene_handle(sc, **opts):
    with R.options(**opts):
        return R.dev_scene(sc, sc.params.spp)


def with_spec(s, spec):
    """rt_dev_scene_set_options: the scene's options with iow_spec = spec (the [build] options stay)."""
    o = R.RtOptions.from_buffer_copy(R.get_options())
    o.iow_spec = spec
    R.check(R.load().rt_dev_scene_set_options(s, C.byref(o)), "rt_dev_scene_set_options")


def fresh(sc_key, spec):
    """The fresh scene's frame, counters and dump for scene_of(*sc_key), computed once."""
    key = ("fresh", sc_key, spec)
    if key not in _cache:
        sc = scene_of(*sc_key)
        s = scene_handle(sc, iow_spec=spec)
        try:
            img, ctr = frame(s, sc)
            _cache[key] = (img, ctr, R.iow_dump(s), R.iow_info(s))
        finally:
            R.load().rt_dev_scene_free(s)
    return _cache[key]


def oracle_frame(sc_key):
    key = ("oracle", sc_key)
    if key not in _cache:
        sc = scene_of(*sc_key)
        rgba, _, st = O.render(sc, sc.params)
        _cache[key] = (rgba.tobytes(), st)
    return _cache[key]


def same_dump(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a["wide"].tobytes() == b["wide"].tobytes() and a["obox"].tobytes() == b["obox"].tobytes()


def on_device(types, rec, offset=0):
    """The types and records as float32 device tensors; offset: the records start `offset` floats into
    their allocation (1: 4 bytes past a 16-byte boundary)."""
    dev = torch.device("cuda")
    d_types = torch.from_numpy(np.ascontiguousarray(types, np.float32)).to(dev)
    flat = torch.from_numpy(np.ascontiguousarray(rec, np.float32).reshape(-1))
    buf = torch.zeros(flat.numel() + offset, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    d_rec = buf[offset:]
    d_rec.copy_(flat)
    torch.cuda.synchronize()
    return d_types, d_rec


def update_dev(s, sc, flags, offset=0):
    d_types, d_rec = on_device(sc.types, sc.records, offset)
    return R.update_iow03_device(s, d_types, d_rec, sc.n, flags)


def expected_built(n, flags, linear=False):
    if linear or n < 2 or n >= 16384 or flags == HOST:
        return 0
    return 1 if flags == DEVICE or n >= DEVICE_BUILD_MIN else 0


def assert_as_fresh(s, key, spec, host_built, what, structures=True):
    """The frame and counters [0], [4], [5] of s are the fresh scene's (and, to 486 objects, the oracle's);
    host_built: all six counters on the sequential kernel and the dump too; otherwise the device-built
    structures are checked directly and the boxes are the host's."""
    sc = scene_of(*key)
    img, ctr = frame(s, sc)
    f_img, f_ctr, f_dump, f_info = fresh(key, spec)
    print(what, "counters", ctr, "fresh", f_ctr, R.iow_info(s))
    assert img == f_img, what
    assert [ctr[k] for k in (0, 4, 5)] == [f_ctr[k] for k in (0, 4, 5)], what
    if sc.n <= N_BASE:
        o_img, o_st = oracle_frame(key)
        assert img == o_img, what
        assert ctr[0] == o_st["segments"], what
    info = R.iow_info(s)
    assert info["objects"] == sc.n
    if host_built:
        # (counters [1] and [2] of the sample-parallel pipeline depend on the device's scheduling: all six
        # are compared on the same handle switched to the sequential kernel)
        if spec:
            with_spec(s, 0)
            try:
                assert frame(s, sc) == fresh(key, 0)[:2], what
            finally:
                with_spec(s, 1)
        else:
            assert ctr == f_ctr, what
        assert same_dump(R.iow_dump(s), f_dump), what
        assert (info["wide_nodes"], info["wide_depth"], info["lds"]) == (
            f_info["wide_nodes"], f_info["wide_depth"], f_info["lds"]), what
    elif structures:
        d = R.iow_dump(s)
        assert d is not None, what
        bad = check_iow_cull(sc.types, sc.records, d["wide"], d["obox"], n_dirs=300 if sc.n <= 2000 else 24)
        assert not bad, (what, bad[:5])
        assert d["obox"].tobytes() == R.iow_host_dump(sc.types, sc.records, sc.n)["obox"].tobytes(), what
    return img


# ---------------------------------------------------------------- records and priors
def record_cases():
    """(name, types, records, linear): every input class of tests/iow_prepare_ref.py, and the sizes at which
    the kernels change path (one object, a wave, a wave + 1, the C2 range, several blocks, the first size
    without a BVH), plain and with the rotation / scale edge rows.  linear: updated on a scene created with
    iow_linear = 1, which builds no BVH -- the rows with a scale of 0 or 1e38 are about the records, not
    about a tree over their boxes."""
    if "record_cases" not in _cache:
        t, r = base().types, base().records
        out = [(name, ct, cr, name == "edges") for name, ct, cr in P.cases(t, r)]
        for n in (1, 2, 3, 64, 65, 485, 1455, 16384):
            out.append((f"tiled{n}", *P.tiled(t, r, n), False))
            if n >= 8:
                out.append((f"edges{n}", *P.edge_rows(t, r, n), True))
        _cache["record_cases"] = out
    return _cache["record_cases"]


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset4"])
def test_records_and_priors_are_the_host_packers(gpu, offset):
    """Hot records, cold records and priors after a device update (the device build where there is a tree:
    the priors then come back with the build's counts) against rt_debug_iow_prepare_host, byte for byte."""
    s = scene_handle(scene_of(5, 0), iow_spec=1)
    lin = scene_handle(scene_of(5, 0), iow_spec=1, iow_linear=1)
    try:
        for name, types, rec, linear in record_cases():
            n = len(types)
            h = lin if linear else s
            d_types, d_rec = on_device(types, rec, offset)
            assert d_rec.data_ptr() % 16 == 4 * offset
            R.update_iow03_device(h, d_types, d_rec, n, DEVICE)
            want, got = R.iow_prepare_host(types, rec), R.iow_records(h)
            print(name, n, "priors", got["priors"], R.iow_info(h))
            assert got["hot"].shape == (n, 20) and got["cold"].shape == (n, 8)
            for k in ("hot", "cold", "priors"):
                assert got[k].tobytes() == want[k].tobytes(), (name, k)
            assert R.iow_info(h)["built"] == expected_built(n, DEVICE, linear), name
    finally:
        R.load().rt_dev_scene_free(s)
        R.load().rt_dev_scene_free(lin)


def test_records_of_a_fresh_scene_and_of_the_host_update(gpu):
    """rt_debug_iow_records on a fresh scene and after rt_dev_scene_iow03_update: the same bytes."""
    a, b = scene_of(485, 0), scene_of(100, 1)
    s = scene_handle(a)
    try:
        for sc in (a, b):
            if sc is b:
                R.update_iow03(s, sc.types, sc.records, 0)
            want, got = R.iow_prepare_host(sc.types, sc.records), R.iow_records(s)
            for k in ("hot", "cold", "priors"):
                assert got[k].tobytes() == want[k].tobytes(), k
    finally:
        R.load().rt_dev_scene_free(s)


# ---------------------------------------------------------------- frames and structures
TRANSITIONS = [((485, 0), (485, 1)), ((485, 0), (100, 1)), ((100, 0), (1455, 1)), ((1455, 0), (3, 1)),
               ((3, 0), (1, 1)), ((1, 0), (2, 1)), ((16383, 0), (16384, 1))]


@pytest.mark.parametrize("spec", [0, 1])
@pytest.mark.parametrize("flags", [HOST, DEVICE, 0])
@pytest.mark.parametrize("a,b", TRANSITIONS, ids=lambda k: f"{k[0]}")
def test_update_matches_fresh_scene(gpu, a, b, flags, spec):
    """A frame of the old scene, the device update, a frame: the fresh scene's (and, to 486 objects, the
    oracle's).  Then back to the first records: the very first frame again.  16383 -> 16384 -> 16383 crosses
    the last BVH size both ways."""
    sa, sb = scene_of(*a), scene_of(*b)
    s = scene_handle(sa, iow_spec=spec)
    try:
        first = assert_as_fresh(s, a, spec, True, f"{a} created")
        for k, (key, sc) in enumerate(((b, sb), (a, sa))):
            tm = update_dev(s, sc, flags)
            print("update ms", tm)
            built = R.iow_info(s)["built"]
            assert built == expected_built(sc.n, flags), (key, flags)
            assert tm[3] >= tm[0] and (built != 1 or tm[2] == 0.0)
            img = assert_as_fresh(s, key, spec, built == 0, f"-> {key} flags {flags}", structures=built == 1)
            assert R.iow_info(s)["updates"] == k + 1
        assert img == first
    finally:
        R.load().rt_dev_scene_free(s)


# ---------------------------------------------------------------- queries and passes
def up(a):
    return torch.from_numpy(np.frombuffer(a.tobytes() + bytes(64), np.uint8).copy()).to(torch.device("cuda"))


def queries(s, sc):
    """Every query family on device scene s, as bytes: 16 pixels' camera rays, the first 64 through the
    closest-hit and any-hit queries, all of them through the path queries in chains of spp, the pixel query
    of 8 pixels, one rt_render_pass_async frame of 2 passes and one rt_render_pass_pixels_async round."""
    lib = R.load()
    p = sc.params
    st = torch.cuda.current_stream().cuda_stream
    dev = torch.device("cuda")
    px = R.as_pixels([(3 * i + 1, 2 * i) for i in range(16)])
    d_px = up(px)
    n = len(px) * p.spp
    d_rays = torch.zeros(n * R.PATH_IOW_RAY_DTYPE.itemsize + 64, dtype=torch.uint8, device=dev)
    assert lib.rt_camera_rays_async(s, C.byref(sc.camera), C.byref(p), d_px.data_ptr(), len(px), 0, p.spp,
                                    d_rays.data_ptr(), st) == R.RT_OK
    torch.cuda.synchronize()
    cam = d_rays.cpu().numpy()[: n * R.PATH_IOW_RAY_DTYPE.itemsize].view(R.PATH_IOW_RAY_DTYPE)
    out = {"camera_rays": cam.tobytes()}
    rays = np.zeros(64, R.RAY_DTYPE)
    rays["o"], rays["d"], rays["tmax"] = cam["o"][:64], cam["d"][:64], 32000.0
    d_q = up(rays)
    for name, flags in (("closest", 0), ("any", R.RT_TRACE_ANY)):
        d_hits = torch.zeros(64 * 32, dtype=torch.uint8, device=dev)
        ctr = torch.zeros(6, dtype=torch.int64, device=dev)
        assert lib.rt_trace_iow_rays_async(s, d_q.data_ptr(), 64, flags, d_hits.data_ptr(), ctr.data_ptr(), st) == R.RT_OK
        torch.cuda.synchronize()
        hits = d_hits.cpu().numpy().view(R.HIT_DTYPE)
        out[name] = (hits["id"] >= 0).tobytes() if flags else hits.tobytes()
        out[name + " rays"] = int(ctr[0])
    d_out = torch.zeros(n * R.PATH_IOW_OUT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    ctr = torch.zeros(6, dtype=torch.int64, device=dev)
    assert lib.rt_path_iow_rays_async(s, d_rays.data_ptr(), n, p.spp, p.max_bounces, 0, d_out.data_ptr(), ctr.data_ptr(),
                                      st) == R.RT_OK
    torch.cuda.synchronize()
    out["paths"] = d_out.cpu().numpy().tobytes()
    out["paths counters"] = [int(ctr[k]) for k in (0, 4, 5)]
    need = lib.rt_pixel_workspace_bytes(s, 8)
    d_ws = torch.zeros(max(need, 16), dtype=torch.uint8, device=dev)
    d_pout = torch.zeros(8 * 32, dtype=torch.uint8, device=dev)
    ctr = torch.zeros(6, dtype=torch.int64, device=dev)
    assert lib.rt_pixel_query_async(s, C.byref(sc.camera), C.byref(p), d_px.data_ptr(), 8, d_pout.data_ptr(), None,
                                    d_ws.data_ptr(), need, ctr.data_ptr(), st) == R.RT_OK
    torch.cuda.synchronize()
    out["pixels"] = d_pout.cpu().numpy().tobytes()
    out["pixels counters"] = [int(ctr[k]) for k in (0, 4, 5)]
    # a progressive frame of two passes, then one adaptive round over the 16 listed pixels
    npx = p.width * p.height
    d_state = torch.zeros(npx * 32, dtype=torch.uint8, device=dev)
    d_rgba = torch.zeros(npx * 16, dtype=torch.uint8, device=dev)
    ctr = torch.zeros(6, dtype=torch.int64, device=dev)
    half = p.spp // 2
    for s0, ns in ((0, half), (half, p.spp - half)):
        assert lib.rt_render_pass_async(s, C.byref(sc.camera), C.byref(p), s0, ns, d_state.data_ptr(), d_rgba.data_ptr(),
                                        None, ctr.data_ptr(), st) == R.RT_OK
    torch.cuda.synchronize()
    out["pass state"] = d_state.cpu().numpy().tobytes()
    out["pass rgba"] = d_rgba.cpu().numpy().tobytes()
    out["pass counters"] = [int(ctr[k]) for k in (0, 4, 5)]
    d_state.zero_()
    d_rgba.zero_()
    d_aux = torch.zeros(npx * 16, dtype=torch.uint8, device=dev)
    ctr = torch.zeros(6, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    assert R.pass_pixels(s, sc.camera, p, d_px, len(px), 2, d_state, d_aux, d_rgba, None, ctr, st) == R.RT_OK
    torch.cuda.synchronize()
    out["pixel pass state"] = d_state.cpu().numpy().tobytes()
    out["pixel pass aux"] = d_aux.cpu().numpy().tobytes()
    out["pixel pass rgba"] = d_rgba.cpu().numpy().tobytes()
    out["pixel pass counters"] = [int(ctr[k]) for k in (0, 4, 5)]
    return out


@pytest.mark.parametrize("flags", [HOST, DEVICE])
@pytest.mark.parametrize("n_new", [485, 1455, 1])
def test_queries_and_passes_match_fresh_scene(gpu, n_new, flags):
    """The query families and the passes after a device update (to a scene with the LDS-staged instances, to
    one past their cap, to one without a BVH): byte-equal to a fresh scene's."""
    sc = scene_of(n_new, 1)
    s = scene_handle(scene_of(300, 0))
    f = scene_handle(sc)
    try:
        update_dev(s, sc, flags)
        got, want = queries(s, sc), queries(f, sc)
        assert any(np.frombuffer(want["closest"], R.HIT_DTYPE)["id"] >= 0)  # the rays do meet the scene
        assert np.frombuffer(want["pass state"], np.float32).any() and np.frombuffer(want["pixel pass aux"], np.uint8).any()
        for k in want:
            assert got[k] == want[k], k
    finally:
        R.load().rt_dev_scene_free(s)
        R.load().rt_dev_scene_free(f)


# ---------------------------------------------------------------- streams
@pytest.mark.parametrize("flags", [HOST, DEVICE])
def test_stream_order(gpu, flags):
    """The records are produced by a torch op on a non-blocking stream, the update follows on that stream
    with no synchronisation in between, and a frame is enqueued on another non-blocking stream right after
    the return: the fresh scene's."""
    old = scene_of(485, 0)
    s = scene_handle(scene_of(100, 0), iow_spec=1)
    try:
        dev = torch.device("cuda")
        d_types, d_old = on_device(old.types, old.records)
        d_delta = torch.from_numpy((scene_of(485, 1).records - old.records).reshape(-1)).to(dev)
        torch.cuda.synchronize()
        prod, other = torch.cuda.Stream(), torch.cuda.Stream()
        with torch.cuda.stream(prod):
            d_rec = d_old + d_delta
            R.update_iow03_device(s, d_types, d_rec, old.n, flags, stream=prod.cuda_stream)
        img, ctr = frame(s, old, stream=other)
        now = with_records(old.types, d_rec.cpu().numpy().reshape(-1, 24))  # (copied back for the comparison only)
        assert now.records.tobytes() != old.records.tobytes()
        f = scene_handle(now, iow_spec=1)
        try:
            f_img, f_ctr = frame(f, now)
        finally:
            R.load().rt_dev_scene_free(f)
        assert img == f_img and [ctr[k] for k in (0, 4, 5)] == [f_ctr[k] for k in (0, 4, 5)]
        assert img != fresh((485, 0), 1)[0]
        assert R.iow_records(s)["hot"].tobytes() == R.iow_prepare_host(now.types, now.records)["hot"].tobytes()
    finally:
        R.load().rt_dev_scene_free(s)


@pytest.mark.parametrize("flags", [DEVICE, 0])
def test_device_to_device_loop(gpu, flags):
    """Five steps of records += delta on the GPU, an update and a frame each: every frame is the frame of a
    fresh scene made from the records copied back (for the comparison only)."""
    sc0 = scene_of(485, 0)
    s = scene_handle(sc0, iow_spec=1)
    try:
        dev = torch.device("cuda")
        d_types, d_rec = on_device(sc0.types, sc0.records)
        delta = np.zeros((sc0.n, 24), np.float32)
        i = np.arange(sc0.n)
        for k in range(3):
            delta[:, k] = 0.02 * ((i + k) % 3 - 1)
        d_delta = torch.from_numpy(delta.reshape(-1)).to(dev)
        st = torch.cuda.current_stream()
        frames = []
        for step in range(5):
            d_rec += d_delta
            R.update_iow03_device(s, d_types, d_rec, sc0.n, flags, stream=st.cuda_stream)
            img, ctr = frame(s, sc0)
            now = with_records(sc0.types, d_rec.cpu().numpy().reshape(-1, 24))
            f = scene_handle(now, iow_spec=1)
            try:
                f_img, f_ctr = frame(f, now)
            finally:
                R.load().rt_dev_scene_free(f)
            assert img == f_img and [ctr[k] for k in (0, 4, 5)] == [f_ctr[k] for k in (0, 4, 5)], step
            frames.append(img)
        assert len(set(frames)) == 5  # the objects did move
        assert R.iow_info(s)["updates"] == 5 and R.iow_info(s)["built"] == expected_built(sc0.n, flags)
    finally:
        R.load().rt_dev_scene_free(s)


# ---------------------------------------------------------------- fallbacks, [build] options, errors
def test_level_cap_falls_back_to_the_host_build(gpu):
    lib = R.load()
    key = (485, 1)
    sc = scene_of(*key)
    s = scene_handle(scene_of(485, 0), iow_spec=1)
    try:
        assert lib.rt_debug_build_level_cap(3) == 0
        try:
            tm = update_dev(s, sc, DEVICE)
        finally:
            lib.rt_debug_build_level_cap(0)
        assert R.iow_info(s)["built"] == 2 and tm[2] > 0.0
        assert_as_fresh(s, key, 1, True, "level cap 3")  # host-built: everything equals the fresh scene's
        want, got = R.iow_prepare_host(sc.types, sc.records), R.iow_records(s)
        for k in ("hot", "cold", "priors"):
            assert got[k].tobytes() == want[k].tobytes(), k
    finally:
        lib.rt_dev_scene_free(s)


@pytest.mark.parametrize("flags", [HOST, DEVICE, 0])
def test_linear_scene_builds_nothing(gpu, flags):
    """A scene created with iow_linear = 1 keeps the linear loop through a device update."""
    key = (100, 1)
    sc = scene_of(*key)
    s = scene_handle(scene_of(485, 0), iow_spec=1, iow_linear=1)
    try:
        tm = update_dev(s, sc, flags)
        info = R.iow_info(s)
        assert (info["objects"], info["wide_nodes"], info["lds"], info["built"]) == (100, 0, 0, 0) and R.iow_dump(s) is None
        assert tm[2] == 0.0
        img, ctr = frame(s, sc)
        f_img, f_ctr, _, _ = fresh(key, 1)
        assert img == f_img and [ctr[k] for k in (0, 4, 5)] == [f_ctr[k] for k in (0, 4, 5)]
        assert img == oracle_frame(key)[0]
    finally:
        R.load().rt_dev_scene_free(s)


def test_wrong_family_and_argument_errors(gpu):
    """An INW handle is RT_E_UNSUPPORTED; an argument error on a live IOW-03 scene leaves it rendering the
    old frame, timing_ms unwritten."""
    lib = R.load()
    key = (100, 0)
    sc, new = scene_of(*key), scene_of(64, 1)
    d_types, d_rec = on_device(new.types, new.records)
    t, r = d_types.data_ptr(), d_rec.data_ptr()
    tm = (C.c_double * 4)(7.0, 7.0, 7.0, 7.0)
    inw = R.make_scene(R.PRESET_INW01_RANDOM, 1234, 50, width=16, height=16, spp=2)
    h = R.dev_scene(inw)
    try:
        assert lib.rt_dev_scene_iow03_update_device(h, t, r, new.n, 0, None, tm) == R.RT_E_UNSUPPORTED
        assert lib.rt_debug_iow_records(h, None, None, (C.c_float * 10)()) == R.RT_E_ARG
        assert list(tm) == [7.0] * 4
    finally:
        lib.rt_dev_scene_free(h)
    s = scene_handle(sc, iow_spec=0)  # (the sequential kernel: all six counters repeat)
    try:
        before = frame(s, sc)
        for a_t, a_r, n, flags in ((None, r, new.n, 0), (t, None, new.n, 0), (t, r, 0, 0), (t, r, new.n, HOST | DEVICE),
                                   (t, r, new.n, 4), (t, r, new.n, -1)):
            assert lib.rt_dev_scene_iow03_update_device(s, a_t, a_r, n, flags, None, tm) == R.RT_E_ARG
        assert list(tm) == [7.0] * 4
        assert lib.rt_debug_walk_dump(s, R.RT_WALK_WNODES, None, 0, (C.c_uint64 * 8)()) == R.RT_E_ARG
        assert R.iow_info(s)["updates"] == 0
        assert frame(s, sc) == before == fresh(key, 0)[:2]
    finally:
        lib.rt_dev_scene_free(s)


def test_kernel_resources(gpu):
    """The new kernels keep their registers: no scratch; k_iow_prepare uses no LDS."""
    for which, name in enumerate(R.UPDATE_IOW_KERNELS):
        info = R.update_iow_kernel_info(which)
        print(name, info)
        assert info["scratch_bytes"] == 0, name
        assert info["vgprs"] > 0 and info["blocks_per_cu"] >= 1, name
        if which < 2:
            assert info["lds_bytes"] == 0, name
