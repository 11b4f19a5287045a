"""What the walk-trip fixtures (tests/golden/trace_walk_*.npz, written by
tests/golden/make_walk_trip_golden.py) must contain, checked on the CPU: by the generator when it
writes them and by tests/test_walk_trip_ref.py.  The GPU test (tests/test_gpu_walk_trip.py) relies
on these cases being there, inside one 64-query wave beside lanes doing something else."""
import ctypes as C

import numpy as np

import rt_amd as R

FIXTURES = ["walk_chain", "walk_pile", "walk_moving", "walk_face", "walk_three", "walk_one"]
CHAIN_N, CHAIN_GROWTH = 47, 1.5
# time ratios of walk_moving: bins 0, 0, 1, 1 of two
RATIOS = np.array([0.0, np.nextafter(np.float32(0.5), np.float32(0.0)), 0.5, 1.0], np.float32)
FACE_MIN_PER_WAVE = 8  # walk_face: hits with t <= their leaf-box entry in every 64-query wave, and as many others
WALK_CAP = 40 - 3  # the query kernel's walk stack: the 40-float stack less 3 slots for branch-free pushes
F = np.float32
MISS = F(np.inf)


def wide_nodes(fx, bins=2):
    """The host-built 4-wide nodes (N, 40) with the links as int32 (N, 4), and rt_debug_time_bins's
    info = (nodes of the swept tree, bins built, nodes per bin tree, all nodes)."""
    lib = R.load()
    geom, nodes = np.ascontiguousarray(fx["geom"], F), np.ascontiguousarray(fx["nodes"], F)
    n = geom.shape[0]
    info = (C.c_uint32 * 4)()
    R.check(lib.rt_debug_time_bins(R.fptr(nodes), R.fptr(geom), n, bins, None, 0, info), "rt_debug_time_bins")
    total = int(info[3])
    wn = np.zeros((max(total, 1), 40), F)
    if total:
        R.check(lib.rt_debug_time_bins(R.fptr(nodes), R.fptr(geom), n, bins, R.fptr(wn), total, info), "rt_debug_time_bins")
    return wn, wn[:, 36:40].copy().view(np.int32), tuple(int(v) for v in info)


def _cswap(t, k, a, b):
    if t[b] < t[a]:
        t[a], t[b], k[a], k[b] = t[b], t[a], k[b], k[a]


def walk_model(wn, links, root, o, d, tmax, cap=WALK_CAP, whole=False):
    """One lane of inw_traverse_wide (unfused cull).  Returns (the walk's stack went past cap, its
    highest stack pointer, node steps).
    whole = False: up to the trip where the lane would wait on a second leaf -- until then no leaf
    has been tested, so the culling limit is the initial one and the lane's stack does not depend
    on the other lanes of its wave: what it returns is what the kernel's lane does (an overflow
    found here happens, after exactly `steps` node steps).
    whole = True: the whole walk with the limit left at its initial value and every leaf taken at
    once.  A leaf test can only lower the limit, a lower limit only culls more children, and the
    children's order does not depend on it, so at every node the kernel's stack holds a subset of
    this one's entries: no overflow here means none in the kernel, whatever the wave does."""
    o, d = o.astype(F), d.astype(F)
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        inv = F(1.0) / d
        lim = F(F(tmax) * F(1.0001) + F(1e-3))
        stack, cur, pend, high, steps = [], root, -1, 0, 0
        while True:
            if cur > 0:
                nd = wn[cur - 1]
                t = []
                for c in range(4):
                    te, tx = F(-np.inf), F(np.inf)
                    for a in range(3):
                        s = 1 if d[a] < 0 else 0
                        near, far = nd[4 * (a + 3 * s) + c], nd[4 * (a + 3 * (1 - s)) + c]
                        te, tx = max(te, F((near - o[a]) * inv[a])), min(tx, F((far - o[a]) * inv[a]))
                    t.append(te if max(te, F(-1e-3)) <= min(tx, lim) else MISS)
                k = [int(v) for v in links[cur - 1]]
                _cswap(t, k, 0, 1); _cswap(t, k, 2, 3); _cswap(t, k, 0, 2); _cswap(t, k, 1, 3); _cswap(t, k, 1, 2)
                steps += 1
                stack += [k[j] for j in (3, 2, 1) if t[j] != MISS]
                high = max(high, len(stack))
                if len(stack) > cap:
                    return True, high, steps
                cur, pop = k[0], t[0] == MISS
            else:
                if pend >= 0 and not whole:
                    return False, high, steps
                pend, pop = -cur, True
            if pop:
                if not stack:
                    return False, high, steps
                cur = stack.pop()


def boxes_crossed(aabbs, o, d):
    """How many of the boxes the ray o + t d, t > 0, passes through (float64 slabs; d has no zero)."""
    o, d = o.astype(np.float64), d.astype(np.float64)
    a, b = (aabbs[:, :3] - o) / d, (aabbs[:, 3:] - o) / d
    te, tx = np.minimum(a, b).max(1), np.maximum(a, b).min(1)
    return int(np.sum((te < tx) & (tx > 0)))


def leaf_entry(box, o, d):
    """test_aabb_te's entry t of a leaf box (the kernels' float operations, in their order)."""
    inv = F(1.0) / d.astype(F)
    te = F(-np.inf)
    for a in range(3):
        p, q = F((box[a] - o[a]) * inv[a]), F((box[3 + a] - o[a]) * inv[a])
        te = min(p, q) if a == 0 else max(min(p, q), te)
    return te


def check(name, fx):
    """Assert the fixture's cases; returns a short summary."""
    rays, geom, n = fx["rays"], fx["geom"], fx["geom"].shape[0]
    info = R.inw_host_build(fx["nodes"], n)
    waves = [slice(w, min(w + 64, len(rays))) for w in range(0, len(rays), 64)]
    o, d = rays["o"], rays["d"]
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        inv = F(1.0) / d
        finite = np.isfinite(inv).all(1) & (d != 0).all(1)
        fused_ok = finite & np.isfinite(-(o * inv)).all(1)
    if name == "walk_chain":
        assert n == CHAIN_N and 0 < info["dfs_high"] <= 40, info  # the walk's own condition holds
        wn, links, (n0, bins, stride, total) = wide_nodes(fx)
        assert bins == 1 and finite.all()
        lanes = np.arange(len(rays)) % 64
        # the row lanes overflow for certain (before their first leaf test); the others cannot
        over = np.array([walk_model(wn, links, 1, o[q], d[q], rays["tmax"][q], whole=lanes[q] >= 16)[0]
                         for q in range(len(rays))])
        assert over[lanes < 16].all() and not over[lanes >= 16].any()
        return {"dfs_high": info["dfs_high"], "wide_depth": info["wide_depth"], "overflowing": int(over.sum())}
    if name == "walk_pile":
        assert 0 < info["dfs_high"] <= 40 and finite.all(), info
        cnt = np.array([boxes_crossed(fx["aabbs"], o[q], d[q]) for q in range(len(rays))])
        # even lanes cross the whole pile, every fourth lane crosses nothing (it is done after the
        # root), the others a scattered sphere and whatever lies on the way
        assert np.all(cnt[0::2] >= 20) and np.all(cnt[3::4] == 0) and np.median(cnt[1::4]) <= 3
        return {"dfs_high": info["dfs_high"], "boxes_even": int(cnt[0::2].min()), "boxes_aimed": int(np.median(cnt[1::4]))}
    if name == "walk_moving":
        assert 0 < info["dfs_high"] <= 40, info
        bins = wide_nodes(fx)[2][1]
        assert bins == 2
        assert np.array_equal(rays["ratio"].reshape(-1, 4), np.tile(RATIOS, (len(rays) // 4, 1)))
        assert [min(int(F(r) * F(2.0)), 1) for r in RATIOS] == [0, 0, 1, 1]
        zero, fus = (d == 0).any(1), finite & ~fused_ok
        infr = (~np.isfinite(inv)).any(1) & ~zero
        assert zero.sum() >= 32 and infr.sum() >= 32 and fus.sum() >= 32
        for w in waves:  # refused lanes beside taken ones in every wave
            assert 4 <= int((~fused_ok[w]).sum()) <= 32
        return {"dfs_high": info["dfs_high"], "bins": bins, "zero": int(zero.sum()), "inf_rcp": int(infr.sum()),
                "fused_overflow": int(fus.sum())}
    if name == "walk_face":
        assert 0 < info["dfs_high"] <= 40 and finite.all(), info
        assert np.array_equal(geom[: n // 2], geom[n // 2:])
        # the host builds sphere records for this scene, so inw_sphere_records = 1 takes the
        # sphere-record leaf test (the C3 frame's) and = 0 the full-record one
        rec = np.zeros((n, 12), F)
        assert R.load().rt_debug_sphere_records(R.fptr(np.ascontiguousarray(geom, F)), n, fx["layout"], R.fptr(rec)) == 1
        out = {}
        for inv_order in (0, 1):
            h = fx[f"hits{inv_order}"]
            at = np.array([h["id"][q] >= 0 and h["t"][q] <= leaf_entry(fx["aabbs"][h["id"][q]], o[q], d[q])
                           for q in range(len(rays))])
            other = (h["id"] >= 0) & ~at
            for w in waves:  # in every wave: hits at or below their leaf-box entry beside ordinary ones
                assert int(at[w].sum()) >= FACE_MIN_PER_WAVE and int(other[w].sum()) >= FACE_MIN_PER_WAVE, \
                    (w, int(at[w].sum()), int(other[w].sum()))
            out[f"t_le_entry{inv_order}"] = int(at.sum())
            out[f"per_wave_min{inv_order}"] = min(int(at[w].sum()) for w in waves)
        return out
    if name == "walk_three":
        wn, links, (n0, bins, stride, total) = wide_nodes(fx)
        assert n == 3 and n0 == 1 and np.all((links[0] <= 0) | (links[0] > 1))  # one node: three leaves, an empty slot
        return {"wide_nodes": n0}
    if name == "walk_one":
        assert n == 1 and fx["nodes"].shape == (1, 8) and not fx["nodes"][0, 6] > 0.1  # the LBVH root is a leaf
        return {"wide_nodes": info["wide_nodes"]}
    raise KeyError(name)
