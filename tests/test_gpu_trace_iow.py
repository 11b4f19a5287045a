"""Batched closest-hit ray queries on IOW-03 scenes (rt_trace_iow_rays_async / rt_trace_iow03) on the
GPU, bit for bit against the fixtures tests/golden/trace_iow_*.npz (the CPU oracle's launch_ray per
query, tests/trace_iow_ref.c; tests/test_trace_iow_ref.py recomputes them): t, id, normal, extra and
the query count, for both entry points, ragged batch sizes on the LDS and the global node path,
every scene option, rebuilt scenes and the occlusion flag."""
import numpy as np
import pytest

import rt_amd as R
import trace_iow_ref as T

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = 0xCD


class _Fx:
    """A fixture as a packed scene (what R.trace_iow takes)."""

    def __init__(self, name):
        d = T.load_fixture(name)
        self.types, self.records = d["types"], d["records"]
        self.n = len(self.types)
        self.rays, self.hits, self.ovf = d["rays"], d["hits"], d["ovf"]


_cache = {}


def fx(name) -> _Fx:
    if name not in _cache:
        _cache[name] = _Fx(name)
    return _cache[name]


def dev_scene(f: _Fx):
    s = R.load().rt_dev_scene_iow03(R.fptr(f.types), R.fptr(f.records), f.n, 1, -1)
    assert s
    return s


def trace_async(s, rays, flags, n_rays=None, cap=None):
    """rt_trace_iow_rays_async on the current torch stream; the hit buffer (cap records) starts as
    SENTINEL bytes.  Returns (rc, hits (cap,), counters (6,))."""
    rays = np.ascontiguousarray(rays, R.RAY_DTYPE)
    n_rays = len(rays) if n_rays is None else n_rays
    cap = max(len(rays), 1) if cap is None else cap
    dev = torch.device("cuda")
    d_rays = torch.from_numpy(np.frombuffer(rays.tobytes() + bytes(32), np.uint8).copy()).to(dev)
    d_hits = torch.full((cap * 32,), SENTINEL, dtype=torch.uint8, device=dev)
    d_ctr = torch.zeros(6, dtype=torch.int64, device=dev)
    rc = R.load().rt_trace_iow_rays_async(s, d_rays.data_ptr(), n_rays, flags, d_hits.data_ptr(), d_ctr.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, d_hits.cpu().numpy().view(R.HIT_DTYPE), d_ctr.cpu().numpy()


def assert_same(got, want, what):
    assert got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero((got.view(np.uint32).reshape(-1, 8) != want.view(np.uint32).reshape(-1, 8)).any(1))
        raise AssertionError(f"{what}: {len(bad)} of {len(got)} hits differ, first {bad[0]}: got {got[bad[0]]} "
                             f"want {want[bad[0]]}")


@pytest.mark.parametrize("name", T.SCENES)
def test_parity_blocking_and_async(gpu, name):
    f = fx(name)
    hits, st = R.trace_iow(f, f.rays)
    assert_same(hits, f.hits, f"{name} rt_trace_iow03")
    assert st["segments"] == len(f.rays)
    assert st["shadow_queries"] == 0 and st["stack_drops"] == 0 and st["nan_drops"] == 0
    s = dev_scene(f)
    try:
        rc, hits, ctr = trace_async(s, f.rays, 0)
    finally:
        R.load().rt_dev_scene_free(s)
    assert rc == R.RT_OK
    assert_same(hits, f.hits, f"{name} rt_trace_iow_rays_async")
    assert ctr[0] == len(f.rays) and not ctr[3:].any()
    assert ctr[2] > 0 and (ctr[1] > 0) == (f.n >= 2)


@pytest.mark.parametrize("name", ["final", "final2"])  # nodes in LDS / in global memory
def test_batch_sizes_and_untouched_tail(gpu, name):
    """Prefixes around the 64-query wave claim: the lanes without a query must neither hang the
    walk's votes nor change the others' answers; hits past n_rays keep the sentinel."""
    f = fx(name)
    s = dev_scene(f)
    try:
        for k in (0, 1, 63, 64, 65, 2047):
            rc, hits, ctr = trace_async(s, f.rays, 0, n_rays=k, cap=len(f.rays))
            assert rc == R.RT_OK, k
            assert_same(hits[:k], f.hits[:k], f"{name} prefix {k}")
            assert np.all(hits[k:].view(np.uint8) == SENTINEL), k
            assert ctr[0] == k and not ctr[3:].any()
    finally:
        R.load().rt_dev_scene_free(s)


@pytest.mark.parametrize("name", ["final", "final2"])
def test_large_batch_claims_several_rounds(gpu, name):
    """Past about 2.1M queries (64 x 4 claims x 4 waves x 1024 blocks x 2) a wave claims more than 64
    queries per atomic and answers them in rounds: the fixture tiled to 3.3M queries and a ragged
    tail, each copy bit for bit, the sentinel tail untouched."""
    f = fx(name)
    reps, tail = 1600, 37
    rays = np.concatenate([np.tile(f.rays, reps), f.rays[:tail]])
    dev = torch.device("cuda")
    d_rays = torch.from_numpy(rays.view(np.uint8)).to(dev)
    d_hits = torch.full(((len(rays) + 64) * 32,), SENTINEL, dtype=torch.uint8, device=dev)
    d_ctr = torch.zeros(6, dtype=torch.int64, device=dev)
    s = dev_scene(f)
    try:
        rc = R.load().rt_trace_iow_rays_async(s, d_rays.data_ptr(), len(rays), 0, d_hits.data_ptr(), d_ctr.data_ptr(),
                                              torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        R.load().rt_dev_scene_free(s)
    assert rc == R.RT_OK
    want = torch.from_numpy(f.hits.view(np.uint8).copy()).to(dev)
    body = d_hits[:reps * len(f.rays) * 32].view(reps, -1)
    assert bool((body == want[None, :]).all())
    assert bool((d_hits[reps * len(f.rays) * 32:len(rays) * 32] == want[:tail * 32]).all())
    assert bool((d_hits[len(rays) * 32:] == SENTINEL).all())
    ctr = d_ctr.cpu().numpy()
    assert ctr[0] == len(rays) and not ctr[3:].any()


OPTIONS = [dict(iow_linear=1), dict(iow_lds_bvh=0), dict(iow_leaf_batch=1), dict(iow_leaf_batch=32),
           dict(iow_leaf_batch=65)]


@pytest.mark.parametrize("option", OPTIONS, ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items()))
@pytest.mark.parametrize("name", ["final", "final2", "rot", "dups", "touch", "shells", "chain"])
def test_options_do_not_change_results(gpu, name, option):
    f = fx(name)
    with R.options(**option):
        hits, st = R.trace_iow(f, f.rays)
        assert_same(hits, f.hits, f"{name} {option}")
        assert st["segments"] == len(f.rays)
        if option.get("iow_linear"):
            # the linear loop tests every object once per query that runs (tmax > 0)
            d = f.rays["d"]
            ok = np.isfinite(d).all(1) & (np.abs(d).sum(1) > 0)
            rays = f.rays[ok | ~(f.rays["tmax"] > 0)]
            hits, st = R.trace_iow(f, rays)
            assert st["node_visits"] == 0
            assert st["prim_tests"] == f.n * int((rays["tmax"] > 0).sum())


def test_rebuilt_scene_after_option_changes(gpu):
    """Trace, change the library options with rt_options_set, build a new scene, trace again."""
    f = fx("final")
    lib = R.load()
    s = dev_scene(f)
    try:
        rc, hits, _ = trace_async(s, f.rays, 0)
        assert rc == R.RT_OK
        assert_same(hits, f.hits, "first scene")
        with R.options(iow_lds_bvh=0, iow_leaf_batch=7):
            s2 = dev_scene(f)
            try:
                rc, hits2, _ = trace_async(s2, f.rays, 0)
            finally:
                lib.rt_dev_scene_free(s2)
            assert rc == R.RT_OK
            assert_same(hits2, f.hits, "second scene, other options")
            rc, hits, _ = trace_async(s, f.rays, 0)  # the first scene keeps the options it was built with
            assert rc == R.RT_OK
            assert_same(hits, f.hits, "first scene again")
    finally:
        lib.rt_dev_scene_free(s)


@pytest.mark.parametrize("name", ["final", "final2", "one", "dups", "touch", "shells", "chain"])
def test_any_hit(gpu, name):
    f = fx(name)
    want = f.hits
    hits, st = R.trace_iow(f, f.rays, R.RT_TRACE_ANY)
    hit = want["id"] >= 0
    assert np.array_equal(hits["id"] >= 0, hit)
    assert np.all(hits["id"][hit] < f.n)
    assert np.all(want["t"][hit] <= hits["t"][hit]) and np.all(hits["t"][hit] < f.rays["tmax"][hit])
    assert np.array_equal(hits["t"][~hit].view(np.uint32), f.rays["tmax"][~hit].view(np.uint32))
    assert np.all(hits["id"][~hit] == -1)
    assert not hits["n"].any() and not hits["extra"].any() and not hits["pad"].any()
    assert st["segments"] == len(f.rays)


def _ovf_queries(f, **options):
    """The fixture's overflow queries as a batch of their own: (object tests, node visits) per query."""
    rays = f.rays[f.ovf]
    assert len(rays) == 256 and np.all(rays["tmax"] > 0)
    with R.options(**options):
        s = dev_scene(f)
    try:
        rc, hits, ctr = trace_async(s, rays, 0)
    finally:
        R.load().rt_dev_scene_free(s)
    assert rc == R.RT_OK
    assert_same(hits, f.hits[f.ovf], "overflow queries")
    print(f"{options}: {ctr[2] / len(rays):.2f} object tests, {ctr[1] / len(rays):.2f} node visits per query, n = {f.n}")
    return ctr[2] / len(rays), ctr[1] / len(rays)


def test_shells_centre_queries(gpu):
    """The queries from the spheres' common centre lie inside every box, so no box is ever culled.
    Measured: 450.0 object tests per query for n = 450 -- the walk reaches every leaf once and its
    stack does NOT overflow (a re-run would add another 450), so this bound holds without a linear
    re-run; test_chain_overflows_both_stacks
    covers the overflow path."""
    f = fx("shells")
    prims, nodes = _ovf_queries(f)
    assert prims >= f.n and nodes > 0


@pytest.mark.parametrize("lds", [1, 0])
def test_chain_overflows_both_stacks(gpu, lds):
    """A walk without overflow reaches each leaf once, so at most n object tests per query; the linear
    re-run after an overflow adds n: more than n proves the overflow path ran, on the 13 usable
    entries of the LDS path and on the 29 of the global path."""
    f = fx("chain")
    prims, nodes = _ovf_queries(f, iow_lds_bvh=lds)
    assert prims > f.n and nodes > 0


def test_errors_on_a_device(gpu):
    lib = R.load()
    f = fx("ref3")
    s = dev_scene(f)
    try:
        for flags in (R.RT_TRACE_INVERT, R.RT_TRACE_INVERT | R.RT_TRACE_ANY, 4, -1):
            rc, hits, ctr = trace_async(s, f.rays[:4], flags)
            assert rc == R.RT_E_ARG and np.all(hits.view(np.uint8) == SENTINEL) and not ctr.any()
        assert lib.rt_trace_iow_rays_async(s, None, 4, 0, None, None, None) == R.RT_E_ARG
        rc, hits, ctr = trace_async(s, f.rays[:4], 0, n_rays=0)            # nothing to do: nothing launched
        assert rc == R.RT_OK and np.all(hits.view(np.uint8) == SENTINEL) and not ctr.any()
        assert lib.rt_trace_iow_rays_async(s, None, 0, 0, None, None, None) == R.RT_OK
        rc, hits, ctr = trace_async(s, f.rays[:4], 0, n_rays=2 ** 31 + 1)
        assert rc == R.RT_E_ARG and np.all(hits.view(np.uint8) == SENTINEL)
    finally:
        lib.rt_dev_scene_free(s)
    sc = R.make_scene(R.PRESET_INW01_RANDOM, 1234, 50, spp=1)
    si = lib.rt_dev_scene_inw(R.fptr(sc.geom), sc.n, sc.layout, R.fptr(sc.nodes), None, 0, 1, -1)
    assert si
    try:
        rc, hits, ctr = trace_async(si, f.rays[:4], 0)
        assert rc == R.RT_E_UNSUPPORTED and np.all(hits.view(np.uint8) == SENTINEL) and not ctr.any()
    finally:
        lib.rt_dev_scene_free(si)


def test_null_counters(gpu):
    f = fx("rot")
    s = dev_scene(f)
    dev = torch.device("cuda")
    try:
        d_rays = torch.from_numpy(np.frombuffer(f.rays.tobytes(), np.uint8).copy()).to(dev)
        d_hits = torch.zeros(len(f.rays) * 32, dtype=torch.uint8, device=dev)
        rc = R.load().rt_trace_iow_rays_async(s, d_rays.data_ptr(), len(f.rays), 0, d_hits.data_ptr(), None,
                                              torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        R.load().rt_dev_scene_free(s)
    assert rc == R.RT_OK
    assert_same(d_hits.cpu().numpy().view(R.HIT_DTYPE), f.hits, "NULL counters")


def test_kernel_resources(gpu):
    """The query kernel as loaded: no scratch; the link stacks of 256 lanes in LDS (16 slots with the
    240 staged nodes of 7 float4, else 32 slots)."""
    for any_hit in (False, True):
        for lds in (False, True):
            info = R.trace_iow_kernel_info(any_hit, lds)
            assert info["scratch_bytes"] == 0
            assert info["lds_bytes"] == (16 * 256 * 2 + 240 * 7 * 16 if lds else 32 * 256 * 2)
            assert 0 < info["vgprs"] <= 128 and info["blocks_per_cu"] >= 1
