"""Batched path (radiance) queries on IOW-03 scenes (rt_path_iow_rays_async / rt_path_iow03) on the
GPU, bit for bit against the fixtures tests/golden/path_iow_*.npz (the CPU oracle's launch_rays per
query on a ray stack that holds the incoming RI state, tests/path_iow_ref.c; tests/test_path_iow_ref.py
recomputes them): the whole 48-byte answers and the reference's three counters, chains against the
host feeding the state forward, ragged batches, lanes that take one chain after another, every scene
option, whole frames folded from chained queries, and graph capture."""
import ctypes as C
import types as pytypes

import numpy as np
import pytest

import path_iow_ref as P
import rt_amd as R
import trace_iow_ref as T

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = 0xCD
REF_COUNTERS = (0, 4, 5)  # segments, dropped pushes, NaN directions: the reference's

_cache = {}


def fx(name):
    """The fixture with its scene (types, records, n) and the reference counters in the ABI's slots."""
    if name not in _cache:
        f = P.load_fixture(name)
        s = T.load_fixture(str(f["scene"]))
        want = np.zeros(6, np.int64)
        want[list(REF_COUNTERS)] = f["ctr"]
        _cache[name] = pytypes.SimpleNamespace(name=name, types=s["types"], records=s["records"], n=len(s["types"]),
                                               rays=f["rays"], out=f["out"], chain=f["chain"],
                                               max_bounces=f["max_bounces"], ctr=want, camera=f.get("camera"))
    return _cache[name]


@pytest.fixture(scope="module")
def ref_lib(tmp_path_factory):
    return P.build(tmp_path_factory.mktemp("path_iow_ref_gpu"))


def dev_scene(f, spp=P.SPP):
    s = R.load().rt_dev_scene_iow03(R.fptr(f.types), R.fptr(f.records), f.n, spp, -1)
    assert s
    return s


def path_async(s, rays, max_bounces, chain, flags=0, n_rays=None, cap=None, counters=True):
    """rt_path_iow_rays_async on the current torch stream; the output buffer (cap records) starts as
    SENTINEL bytes.  Returns (rc, out (cap,), counters (6,))."""
    rays = np.ascontiguousarray(rays, R.PATH_IOW_RAY_DTYPE)
    n_rays = len(rays) if n_rays is None else n_rays
    cap = max(len(rays), 1) if cap is None else cap
    dev = torch.device("cuda")
    d_rays = torch.from_numpy(np.frombuffer(rays.tobytes() + bytes(48), np.uint8).copy()).to(dev)
    d_out = torch.full((cap * 48,), SENTINEL, dtype=torch.uint8, device=dev)
    d_ctr = torch.zeros(6, dtype=torch.int64, device=dev)
    rc = R.load().rt_path_iow_rays_async(s, d_rays.data_ptr(), n_rays, chain, max_bounces, flags, d_out.data_ptr(),
                                         d_ctr.data_ptr() if counters else None,
                                         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, d_out.cpu().numpy().view(R.PATH_IOW_OUT_DTYPE), d_ctr.cpu().numpy()


def assert_same(got, want, what):
    """Bit for bit, but for which NaN an rgb of a NaN-direction query is (P.canon)."""
    assert got.shape == want.shape, what
    got, want = P.canon(got), P.canon(want)
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero((got.view(np.uint32).reshape(-1, 12) != want.view(np.uint32).reshape(-1, 12)).any(1))
        raise AssertionError(f"{what}: {len(bad)} of {len(got)} answers differ, first {bad[0]}: got {got[bad[0]]} "
                             f"want {want[bad[0]]}")


def assert_ref_counters(ctr, want, what):
    for k in REF_COUNTERS:
        assert int(ctr[k]) == int(want[k]), (what, k, int(ctr[k]), int(want[k]))
    assert int(ctr[3]) == 0, what


def stats_list(st):
    return [st[k] for k in ("segments", "node_visits", "prim_tests", "shadow_queries", "stack_drops", "nan_drops")]


@pytest.mark.parametrize("name", P.SETS)
def test_parity_blocking_and_async(gpu, name):
    f = fx(name)
    out, st = R.path_iow(f, f.rays, f.max_bounces, f.chain, spp=P.SPP)
    assert_same(out, f.out, f"{name} rt_path_iow03")
    assert_ref_counters(stats_list(st), f.ctr, f"{name} rt_path_iow03")
    assert st["prim_tests"] > 0
    s = dev_scene(f)
    try:
        rc, out, ctr = path_async(s, f.rays, f.max_bounces, f.chain)
    finally:
        R.load().rt_dev_scene_free(s)
    assert rc == R.RT_OK
    assert_same(out, f.out, f"{name} rt_path_iow_rays_async")
    assert_ref_counters(ctr, f.ctr, f"{name} rt_path_iow_rays_async")
    assert ctr[2] > 0 and (ctr[1] > 0) == (name != "one")  # `one` has no BVH


def test_chain_is_the_host_feeding_the_state_forward(gpu):
    """final as eight launches of 600 independent queries, each taking the ri_out of the one before."""
    f = fx("final")
    rays = f.rays.reshape(-1, 8).copy()
    want = f.out.reshape(-1, 8)
    state = rays["ri_in"][:, 0].copy()
    s = dev_scene(f)
    try:
        for j in range(8):
            step = rays[:, j].copy()
            step["ri_in"] = state
            rc, out, _ = path_async(s, step, f.max_bounces, 1)
            assert rc == R.RT_OK
            assert_same(out, want[:, j].copy(), f"sample {j}")
            state = out["ri_out"].copy()
    finally:
        R.load().rt_dev_scene_free(s)


@pytest.mark.parametrize("chain", [1, 3, 8])
def test_batch_sizes_and_untouched_tail(gpu, ref_lib, chain):
    """Batches around the 64-chain wave claim, the last chain short; records past n_rays keep the sentinel."""
    f = fx("rot")
    rays = np.tile(f.rays, 2)[:4097 + 7]
    s = dev_scene(f)
    try:
        for k in (1, 63, 64, 65, 4097):
            want, wctr = P.run(ref_lib, f.types, f.records, rays[:k], f.max_bounces, chain)
            rc, out, ctr = path_async(s, rays, f.max_bounces, chain, n_rays=k)
            assert rc == R.RT_OK, k
            assert_same(out[:k], want, f"{k} queries in chains of {chain}")
            assert np.all(out[k:].view(np.uint8) == SENTINEL), k
            assert (ctr[0], ctr[4], ctr[5]) == tuple(int(x) for x in wctr), k
    finally:
        R.load().rt_dev_scene_free(s)


@pytest.mark.parametrize("name", ["rot", "final_deep"])
def test_one_block_refills_its_lanes(gpu, name):
    """A grid of one block: every lane takes several chains, one after another."""
    f = fx(name)
    rays, want, reps = f.rays, f.out, 1
    if name == "final_deep":  # 64 chains are fewer than one block has lanes: six copies
        rays, want, reps = np.tile(f.rays, 6), np.tile(f.out, 6), 6
    assert len(rays) // f.chain > 256
    lib = R.load()
    s = dev_scene(f)
    assert lib.rt_debug_path_iow_max_blocks(1) == 0
    try:
        rc, out, ctr = path_async(s, rays, f.max_bounces, f.chain)
        assert rc == R.RT_OK
        assert_same(out, want, f"{name} one block")
        assert_ref_counters(ctr, f.ctr * reps, f"{name} one block")
    finally:
        assert lib.rt_debug_path_iow_max_blocks(0) == 1
        lib.rt_dev_scene_free(s)


def test_full_grid_refills_its_lanes(gpu):
    """final tiled to twice as many chains as the chip has resident lanes: every tile equals the fixture."""
    f = fx("final")
    cus = C.c_int(0)
    assert R.load().rt_device_info(-1, None, 0, C.byref(cus)) == R.RT_OK and cus.value > 0
    lanes = cus.value * R.path_iow_kernel_info(lds=True)["blocks_per_cu"] * 256
    chains = len(f.rays) // f.chain
    reps = (2 * lanes + chains - 1) // chains
    rays = np.tile(f.rays, reps)
    s = dev_scene(f)
    try:
        rc, out, ctr = path_async(s, rays, f.max_bounces, f.chain)
    finally:
        R.load().rt_dev_scene_free(s)
    assert rc == R.RT_OK
    tiles = out.view(np.uint32).reshape(reps, -1)
    bad = np.flatnonzero((tiles != f.out.view(np.uint32).reshape(1, -1)).any(1))
    assert len(bad) == 0, f"{len(bad)} of {reps} tiles differ, first {bad[0]}"
    assert_ref_counters(ctr, f.ctr * reps, "tiled batch")


@pytest.mark.parametrize("option", [{"iow_linear": 1}, {"iow_lds_bvh": 0}, {"iow_leaf_batch": 1},
                                    {"iow_leaf_batch": 65}], ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
@pytest.mark.parametrize("name", ["final", "rot", "shells"])
def test_options_do_not_change_results(gpu, name, option):
    f = fx(name)
    with R.options(**option):
        s = dev_scene(f)  # a scene keeps the options it was created with
    try:
        rc, out, ctr = path_async(s, f.rays, f.max_bounces, f.chain)
    finally:
        R.load().rt_dev_scene_free(s)
    assert rc == R.RT_OK
    assert_same(out, f.out, f"{name} {option}")
    assert_ref_counters(ctr, f.ctr, f"{name} {option}")
    if "iow_linear" in option:
        assert ctr[1] == 0 and ctr[2] == f.n * ctr[0]  # no nodes, every object per segment


@pytest.mark.parametrize("spec", [1, 0])
def test_a_frame_is_the_fold_of_its_chained_queries(gpu, spec):
    """cam_final's camera rays in chains of spp, folded on the host as out_Pixel folds them, are the GPU
    render of the same 16 x 9 frame bit for bit, by the speculative pipeline and by the sequential one."""
    f = fx("cam_final")
    sc = R.make_scene(R.PRESET_IOW03_FINAL, 20250131, 0, width=P.CAM_W, height=P.CAM_H, spp=P.SPP)
    assert np.array_equal(sc.records, f.records) and sc.params.max_bounces == f.max_bounces
    c = sc.camera
    assert P.same(np.array([*c.pos, *c.dir, c.fov_y_rad, c.aperture, c.focus_dist], np.float32), f.camera)
    out, pst = R.path_iow(f, f.rays, f.max_bounces, P.SPP, spp=P.SPP)
    assert_same(out, f.out, "cam_final")
    with R.options(iow_spec=spec):
        rgba, _, st = R.render(sc)
    assert P.same(P.fold(out, P.SPP), rgba[..., :3].reshape(-1, 3).copy())
    assert st["segments"] == int(out["segments"].sum()) == pst["segments"]
    assert st["stack_drops"] == int(out["drops"].sum()) and st["nan_drops"] == int(out["nans"].sum())


def test_invalid_samples_and_odd_directions(gpu):
    """state: sample >= spp answers status 1 with the state passed through; zero, NaN and non-unit
    directions go where the renders send them.  A batch of invalid samples alone launches and counts
    nothing."""
    f = fx("state")
    bad = f.out["status"] == 1
    assert bad.sum() == 24 and np.all(f.rays["sample"][bad] >= P.SPP)
    s = dev_scene(f)
    try:
        rc, out, ctr = path_async(s, f.rays, f.max_bounces, 1)
        assert rc == R.RT_OK
        assert_same(out, f.out, "state")
        assert not out[bad].view(np.uint32).reshape(-1, 12)[:, :7].any()
        assert np.array_equal(out["ri_out"][bad].view(np.uint32), f.rays["ri_in"][bad].view(np.uint32))
        only = np.tile(f.rays[bad], 11)  # 264 queries: more than a block's lanes
        for chain in (1, 5):
            rc, out, ctr = path_async(s, only, f.max_bounces, chain)
            assert rc == R.RT_OK and np.all(out["status"] == 1) and not ctr.any()
            assert not out.view(np.uint32).reshape(-1, 12)[:, :7].any()
            first = (np.arange(len(only)) // chain) * chain  # the state of a chain's first query passes down it
            assert np.array_equal(out["ri_out"].view(np.uint32), only["ri_in"][first].view(np.uint32))
    finally:
        R.load().rt_dev_scene_free(s)


def test_errors_on_a_device(gpu):
    lib = R.load()
    f = fx("one")
    s = dev_scene(f)
    try:
        assert path_async(s, f.rays[:4], 8, 0)[0] == R.RT_E_ARG              # chain == 0
        assert path_async(s, f.rays[:4], 8, 1, flags=1)[0] == R.RT_E_ARG     # flags are reserved
        assert path_async(s, f.rays[:4], -1, 1)[0] == R.RT_E_ARG             # max_bounces < 0
        assert lib.rt_path_iow_rays_async(s, None, 4, 1, 8, 0, None, None, None) == R.RT_E_ARG
        assert lib.rt_path_iow_rays_async(s, None, (1 << 31) + 1, 1, 8, 0, None, None, None) == R.RT_E_ARG
        rc, out, ctr = path_async(s, f.rays[:4], 8, 1, n_rays=0)              # nothing to do: nothing launched
        assert rc == R.RT_OK and np.all(out.view(np.uint8) == SENTINEL) and not ctr.any()
        assert lib.rt_path_iow_rays_async(s, None, 0, 1, 8, 0, None, None, None) == R.RT_OK
        rc, out, ctr = path_async(s, f.rays, f.max_bounces, f.chain, counters=False)  # null counters
        assert rc == R.RT_OK and not ctr.any()
        assert_same(out, f.out, "NULL counters")
    finally:
        lib.rt_dev_scene_free(s)
    g = R.make_scene(R.PRESET_INW01_RANDOM, 1234, 50, spp=1)
    s1 = lib.rt_dev_scene_inw(R.fptr(g.geom), g.n, g.layout, R.fptr(g.nodes), None, 0, 1, -1)
    assert s1
    try:
        assert path_async(s1, f.rays[:4], 8, 1)[0] == R.RT_E_UNSUPPORTED
    finally:
        lib.rt_dev_scene_free(s1)


def test_graph_capture(gpu):
    """One call captured in a graph (a memset and a kernel on one stream: a single branch), replayed
    twice: the fixture both times, the counters added twice."""
    f = fx("final")
    lib = R.load()
    dev = torch.device("cuda")
    s = dev_scene(f)
    try:
        d_rays = torch.from_numpy(np.frombuffer(f.rays.tobytes(), np.uint8).copy()).to(dev)
        d_out = torch.full((len(f.rays) * 48,), SENTINEL, dtype=torch.uint8, device=dev)
        d_ctr = torch.zeros(6, dtype=torch.int64, device=dev)

        def call():
            return lib.rt_path_iow_rays_async(s, d_rays.data_ptr(), len(f.rays), f.chain, f.max_bounces, 0,
                                              d_out.data_ptr(), d_ctr.data_ptr(),
                                              torch.cuda.current_stream().cuda_stream)

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):  # once outside the capture (the occupancy query runs here)
            assert call() == R.RT_OK
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        d_ctr.zero_()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            assert call() == R.RT_OK
        for k in (1, 2):
            d_out.fill_(SENTINEL)
            graph.replay()
            torch.cuda.synchronize()
            assert_same(d_out.cpu().numpy().view(R.PATH_IOW_OUT_DTYPE), f.out, f"replay {k}")
            assert_ref_counters(d_ctr.cpu().numpy(), f.ctr * k, f"replay {k}")
        del graph
    finally:
        torch.cuda.synchronize()
        lib.rt_dev_scene_free(s)


def test_kernel_resources(gpu):
    """The kernel as loaded: no scratch, and the LDS and registers profiles/path_iow_kres.txt records --
    per 256-lane block the ray stacks (36 floats a lane), the link stacks (16 or 32 shorts a lane) and,
    staged, 240 nodes of 7 float4."""
    table = {True: (136, 36 * 256 * 4 + 16 * 256 * 2 + 240 * 7 * 16), False: (140, 36 * 256 * 4 + 32 * 256 * 2)}
    for lds, (vgprs, lds_bytes) in table.items():
        info = R.path_iow_kernel_info(lds)
        print("k_iow_paths", "lds" if lds else "global", info)
        assert info["scratch_bytes"] == 0
        assert info["lds_bytes"] == lds_bytes and info["vgprs"] == vgprs
        assert info["blocks_per_cu"] >= 1
