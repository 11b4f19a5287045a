"""A plain checker for the culling and bookkeeping structures ("a culling structure may
have any shape, because it only ever rejects work the reference would also reject"): the 4-wide swept
tree and its time-bin trees, their compact and quantised forms, the leaf boxes, the depth-first ranks
and the stack high-water mark, the surrounding-RI grid, and the IOW-03 culling BVH with its object
boxes.  numpy only; it shares no code with the library.  Arithmetic is done in float64 and compared
exactly; where the kernels compare float32 values, so does the checker.  No comparison has a tolerance.

Every check returns a list of (kind, detail) violations instead of asserting, so that
tests/test_walk_structs.py can show that each one reports what it is for.

Node layout (wide nodes, 40 floats = 10 float4): rows 0..2 the four children's low planes x y z, rows
3..5 their high planes, rows 6..8 the low planes again, row 9 the links as int bits: > 0 node index + 1,
<= 0 minus the object id, EMPTY (the int 1000000000) an empty slot whose planes mean nothing.
"""
import numpy as np

EMPTY = 1000000000
F32 = np.float32


def links_of(wnodes):
    return np.ascontiguousarray(wnodes[:, 36:40]).view(np.int32)


def planes_of(wnodes):
    """(nodes, 6, 4) float32: rows 0..5 of the node."""
    return np.ascontiguousarray(wnodes[:, 0:24]).reshape(-1, 6, 4)


def swept_boxes(leafbox):
    """The culling box of each object over its LBVH leaf box (leafbox (n, 8): lo xyz, hi xyz, ...), by
    the formula of k_leaves / inw_wide_build, e = (hi - lo) * 1e-3 + 1e-3 + big * 1e-5 with big the
    largest |coordinate| of the leaf box, evaluated in float32 in the builders' operation order (both
    are compiled without contraction, so numpy float32 gives their bits).

    Why float32 and not float64: the builders store RN32(lo - e) and RN32(hi + e).  Rounding to nearest
    lands inside the float64 box about every other time (host build: 1832 of the 3600 planes of the
    600-object random scene, by up to 1.9e-6; 1848 of 3600 with the scene moved to +-990, by up to
    3.1e-5), so "the stored planes contain the float64 box" fails on correct output; that violation is
    only apparent.  What DESIGN.md §2 needs from the inflation is "e >= 1e-3" (the fused cull's error bound
    is 1.8e-4 |1/d| against it), and the rounding cannot take that away: e holds big * 1e-5, over a
    hundred times the rounding of the subtraction.  So the check is split in two exact ones: the leaf
    slot contains these float32 boxes (a plane one ulp too tight fails), and, in float64, every leaf
    slot plane lies at least 1e-3 outside the leaf box (check_wide_tree's `inner` argument)."""
    b = np.ascontiguousarray(leafbox[:, 0:6], F32)
    big = np.abs(b).max(axis=1).astype(F32)
    out = np.zeros_like(b)
    for k in range(3):
        e = ((b[:, 3 + k] - b[:, k]) * F32(1e-3) + F32(1e-3)).astype(F32) + (big * F32(1e-5)).astype(F32)
        e = e.astype(F32)
        out[:, k] = b[:, k] - e
        out[:, 3 + k] = b[:, 3 + k] + e
    return out


def _tree(planes, links, root, n, obj_boxes, n_nodes=None, depth=None, wbound=None, inner=None, inner_margin=0.0):
    """The tree checks on planes (N, 6, 4) and links (N, 4); root is a link (node index + 1)."""
    v = []
    N = len(planes)
    seen = np.zeros(n, np.int64)
    if not (0 < root <= N):
        return [("link", f"root link {root} outside 1..{N}")]
    levels = [[root - 1]]
    visited = np.zeros(N, bool)
    visited[root - 1] = True
    amax = 0.0
    while levels[-1]:
        nxt = []
        for cur in levels[-1]:
            for k in range(4):
                l = int(links[cur, k])
                if l == EMPTY:
                    continue
                lo, hi = planes[cur, 0:3, k], planes[cur, 3:6, k]
                amax = max(amax, float(np.abs(planes[cur, :, k]).max()))
                if not (lo <= hi).all():
                    v.append(("nest", f"node {cur} slot {k}: lo > hi"))
                if l > 0:
                    if l > N:
                        v.append(("link", f"node {cur} slot {k}: node link {l} > {N}"))
                        continue
                    ch = l - 1
                    if visited[ch]:
                        v.append(("link", f"node {ch} linked twice"))
                        continue
                    visited[ch] = True
                    if ch <= cur:
                        v.append(("order", f"child {ch} of node {cur} is not numbered after it"))
                    live = links[ch] != EMPTY
                    if not live.any():
                        v.append(("link", f"node {ch} is linked but empty"))
                    if not ((planes[ch, 0:3][:, live] >= lo[:, None]).all() and
                            (planes[ch, 3:6][:, live] <= hi[:, None]).all()):
                        v.append(("nest", f"node {ch} does not nest in slot {k} of node {cur}"))
                    nxt.append(ch)
                else:
                    g = -l
                    if g >= n:
                        v.append(("link", f"node {cur} slot {k}: object {g} >= {n}"))
                        continue
                    seen[g] += 1
                    ob = obj_boxes[g]
                    if not ((lo <= ob[0:3]).all() and (hi >= ob[3:6]).all()):
                        v.append(("leaf_box", f"node {cur} slot {k}: leaf slot does not contain object {g}'s box"))
                    if inner is not None:
                        ib = inner[g].astype(np.float64)
                        if not ((lo.astype(np.float64) <= ib[0:3] - inner_margin).all() and
                                (hi.astype(np.float64) >= ib[3:6] + inner_margin).all()):
                            v.append(("margin", f"node {cur} slot {k}: less than {inner_margin} around object {g}"))
        levels.append(nxt)
    levels.pop()
    for g in np.flatnonzero(seen != 1):
        v.append(("reach", f"object {g} reached {seen[g]} times"))
    # breadth first: level L's nodes are the next len(L) indices after level L - 1's
    at = root - 1
    for L, lv in enumerate(levels):
        if sorted(lv) != list(range(at, at + len(lv))):
            v.append(("order", f"level {L} is not the contiguous range from node {at}"))
        at += len(lv)
    count = sum(len(lv) for lv in levels)
    if n_nodes is not None and count != n_nodes:
        v.append(("count", f"{count} reachable nodes, reported {n_nodes}"))
    if depth is not None and len(levels) != depth:
        v.append(("count", f"{len(levels)} levels, reported depth {depth}"))
    if wbound is not None and not (float(wbound) >= amax):
        v.append(("wbound", f"wbound {wbound} < largest |plane| {amax}"))
    return v


def check_wide_tree(wnodes, root, n, obj_boxes, n_nodes=None, depth=None, wbound=None, inner=None,
                    inner_margin=1e-3):
    """The tree under link `root` of wnodes (N, 40): every object reached exactly once ("reach"), valid
    links ("link"), slots nest ("nest"), each leaf slot contains obj_boxes[id] in exact float32
    comparison ("leaf_box"), rows 6..8 repeat rows 0..2 bitwise ("repeat"), breadth-first numbering
    ("order"), node count and depth as reported ("count", where given), wbound at least every |plane| of
    a non-empty slot ("wbound", where given).  inner (n, 6), where given: every leaf slot plane lies at
    least inner_margin outside inner[id] in float64 ("margin"; see swept_boxes)."""
    wn = np.ascontiguousarray(wnodes, F32)
    v = []
    a, b = wn[:, 0:12].view(np.uint32), wn[:, 24:36].view(np.uint32)
    for w in np.flatnonzero((a != b).any(axis=1)):
        v.append(("repeat", f"node {w}: rows 6..8 differ from rows 0..2"))
    return v + _tree(planes_of(wn), links_of(wn), root, n, np.asarray(obj_boxes), n_nodes, depth, wbound, inner,
                     inner_margin)


def check_compact(wnodes, cnodes):
    """Rows 0..5 and row 9 of each wide node appear bitwise in the compact node (cnodes (N, 28))."""
    wn = np.ascontiguousarray(wnodes, F32).view(np.uint32)
    cn = np.ascontiguousarray(cnodes, F32).view(np.uint32)
    if cn.shape != (len(wn), 28):
        return [("compact", f"shape {cn.shape} for {len(wn)} wide nodes")]
    bad = (cn[:, 0:24] != wn[:, 0:24]).any(axis=1) | (cn[:, 24:28] != wn[:, 36:40]).any(axis=1)
    return [("compact", f"node {w} differs from its wide node") for w in np.flatnonzero(bad)]


def unpack_qnodes(qnodes):
    """origin (N, 3), scale (N, 3) float32, low and high bytes (N, 3, 4) int, links (N, 4) int32 of
    qnodes (N, 16): (o.xyz, s.x) (s.y, s.z, qlo.x, qlo.y) (qlo.z, qhi.xyz) links; slot k is byte k."""
    q = np.ascontiguousarray(qnodes, F32)
    u = q.view(np.uint32)
    org, scl = q[:, 0:3], q[:, 3:6]
    sh = np.arange(4, dtype=np.uint32) * 8
    qlo = ((u[:, 6:9, None] >> sh) & 255).astype(np.int64)
    qhi = ((u[:, 9:12, None] >> sh) & 255).astype(np.int64)
    return org, scl, qlo, qhi, u[:, 12:16].view(np.int32)


def check_quantised(wnodes, qnodes, margin):
    """Each quantised node against the wide node it came from.  In float64, per node, axis and
    non-empty slot: o + qlo s <= lo - margin and o + qhi s >= hi + margin ("qplane"); s >= 1e-4
    ("qscale"); empty slots have low byte 255 and high byte 0 ("qempty"); the links are bitwise the wide
    node's ("qlink").  The float32 decode fma(q, s, o) (q s is exact in float64, so float32(q s + o) is
    the fused result) still contains the unmargined planes ("qdecode").  That last check covers the
    decode alone, not the walk's full 1/d form fma(q, s / d, (o - origin) / d), whose error bound
    DESIGN.md §2 derives."""
    wn = np.ascontiguousarray(wnodes, F32)
    if np.asarray(qnodes).shape != (len(wn), 16):
        return [("qplane", f"shape {np.asarray(qnodes).shape} for {len(wn)} wide nodes")]
    org, scl, qlo, qhi, qlk = unpack_qnodes(qnodes)
    lk = links_of(wn)
    pl = planes_of(wn)
    v = []
    for w in np.flatnonzero((qlk != lk).any(axis=1)):
        v.append(("qlink", f"node {w}: links differ"))
    m = float(margin)
    o64, s64 = org.astype(np.float64)[:, :, None], scl.astype(np.float64)[:, :, None]
    dlo, dhi = o64 + qlo * s64, o64 + qhi * s64  # (N, 3, 4), exact products
    lo, hi = pl[:, 0:3].astype(np.float64), pl[:, 3:6].astype(np.float64)
    live = (lk != EMPTY)[:, None, :]
    bad = live & ((dlo > lo - m) | (dhi < hi + m))
    for w, a, k in zip(*np.nonzero(bad)):
        v.append(("qplane", f"node {w} axis {a} slot {k}: decoded plane inside the margined box"))
    anylive = (lk != EMPTY).any(axis=1)
    for w, a in zip(*np.nonzero((scl.astype(np.float64) < 1e-4) & anylive[:, None])):
        v.append(("qscale", f"node {w} axis {a}: scale {scl[w, a]} < 1e-4"))
    bad = ~live & ((qlo != 255) | (qhi != 0))
    for w, a, k in zip(*np.nonzero(bad)):
        v.append(("qempty", f"node {w} axis {a} slot {k}: empty slot bytes ({qlo[w, a, k]}, {qhi[w, a, k]})"))
    flo, fhi = dlo.astype(F32), dhi.astype(F32)
    bad = live & ((flo > pl[:, 0:3]) | (fhi < pl[:, 3:6]))
    for w, a, k in zip(*np.nonzero(bad)):
        v.append(("qdecode", f"node {w} axis {a} slot {k}: float32 decode inside the wide node's plane"))
    return v


def lbvh_leaves(lbvh_nodes, n):
    """Node index of each object's leaf (-1: none) in the LBVH node buffer ((2n-1, 8): lo xyz, hi xyz,
    first child (or minus the object id for a leaf), parent)."""
    nodes = np.asarray(lbvh_nodes, F32)
    leaf = np.full(n, -1, np.int64)
    for i in range(len(nodes)):
        left = nodes[i, 6]
        if not left > 0.1:
            g = int(-left)
            if 0 <= g < n:
                leaf[g] = i
    return leaf


def check_leafboxes(lbvh_nodes, wleaf, n):
    """wleaf (n, 8) is bitwise the LBVH leaf node of each object."""
    nodes = np.ascontiguousarray(lbvh_nodes, F32)
    leaf = lbvh_leaves(nodes, n)
    if np.asarray(wleaf).shape != (n, 8):
        return [("leafbox", f"shape {np.asarray(wleaf).shape} for {n} objects")]
    v = [("leafbox", f"object {g} has no LBVH leaf") for g in np.flatnonzero(leaf < 0)]
    ok = leaf >= 0
    bad = (nodes[leaf[ok]].view(np.uint32) != np.ascontiguousarray(wleaf, F32)[ok].view(np.uint32)).any(axis=1)
    return v + [("leafbox", f"object {g}: not its LBVH leaf node") for g in np.flatnonzero(ok)[bad]]


def lbvh_dfs(lbvh_nodes, n):
    """The reference walk's order over the LBVH (01_BVH shader: push(invert ? right : left),
    push(invert ? left : right), pop from the top, so invert = 0 visits the right child first): rank
    (2, n) of each object for invert 0 and 1, and the most entries the stack ever held."""
    nodes = np.asarray(lbvh_nodes, F32)
    rank = np.full((2, n), -1, np.int64)
    high = 0
    for inv in range(2):
        st, r, high = [0], 0, max(high, 1)
        while st:
            i = st.pop()
            left = nodes[i, 6]
            if left > 0.1:
                l = int(left)
                st += [l + 1, l] if inv else [l, l + 1]
                high = max(high, len(st))
            else:
                rank[inv, int(-left)] = r
                r += 1
    return rank, high


def check_ranks(lbvh_nodes, n, rank, dfs_high):
    """rank (2, n) and dfs_high equal a Python depth-first walk of the LBVH ("rank", "dfs_high")."""
    want, high = lbvh_dfs(lbvh_nodes, n)
    v = []
    got = np.asarray(rank).reshape(2, n).astype(np.int64)
    for inv, g in zip(*np.nonzero(got != want)):
        v.append(("rank", f"invert {inv} object {g}: rank {got[inv, g]}, the walk gives {want[inv, g]}"))
    if int(dfs_high) != high:
        v.append(("dfs_high", f"dfs_high {dfs_high}, the walk's stack holds up to {high}"))
    return v


def ri_cell_of(p, lo, inv, dim):
    """The cell of points p (P, 3) as inw_ri_grid computes it: float32 (p - lo) * inv, truncated,
    clamped; (P,) flat index (z * dim_y + y) * dim_x + x."""
    p = np.asarray(p, F32)
    c = ((p - np.asarray(lo, F32)).astype(F32) * np.asarray(inv, F32)).astype(F32)
    d = np.asarray(dim, np.int64)
    c = np.clip(np.trunc(c.astype(np.float64)), 0, d - 1).astype(np.int64)
    return (c[:, 2] * d[1] + c[:, 1]) * d[0] + c[:, 0]


def ri_points(wleaf, lo, hi, inv, dim, seed=1, uniform=3000, per_boundary=6):
    """Adversarial points for check_ri_grid: every leaf-box corner and face centre with its nextafter
    neighbours inward and outward, points on every cell boundary of each axis +-1 ulp, uniform points."""
    rng = np.random.default_rng(seed)
    b = np.asarray(wleaf, F32)[:, 0:6]
    blo, bhi = b[:, 0:3], b[:, 3:6]
    mid = ((blo.astype(np.float64) + bhi) / 2).astype(F32)
    pts = []
    for cx in range(2):
        for cy in range(2):
            for cz in range(2):
                sel = np.array([cx, cy, cz], bool)
                c = np.where(sel, bhi, blo)
                pts += [c, np.nextafter(c, mid), np.nextafter(c, np.where(sel, F32(np.inf), F32(-np.inf)))]
    for a in range(3):
        for side, face in ((0, blo), (1, bhi)):
            c = mid.copy()
            c[:, a] = face[:, a]
            i, o = c.copy(), c.copy()
            i[:, a] = np.nextafter(face[:, a], mid[:, a])
            o[:, a] = np.nextafter(face[:, a], F32(np.inf if side else -np.inf))
            pts += [c, i, o]
    lo, hi, inv = (np.asarray(x, F32) for x in (lo, hi, inv))
    for a in range(3):
        k = np.arange(int(dim[a]) + 1, dtype=np.float64)
        x = (lo[a] + k / np.float64(inv[a])).astype(F32)
        x = np.concatenate([x, np.nextafter(x, F32(np.inf)), np.nextafter(x, F32(-np.inf))])
        x = np.repeat(x, per_boundary)
        p = rng.uniform(lo.astype(np.float64), hi.astype(np.float64), (len(x), 3)).astype(F32)
        p[:, a] = x
        pts.append(p)
    pts.append(rng.uniform(lo.astype(np.float64), hi.astype(np.float64), (uniform, 3)).astype(F32))
    return np.concatenate(pts).astype(F32)


def check_ri_grid(wleaf, n, cells, ids, lo, hi, inv, dim, points):
    """The surrounding-RI grid against brute force: for each point inside the float bounds (closed
    float32 comparisons, inw_ri_grid's), every object whose leaf box contains the point (closed float32
    comparisons, the walk's own test in rt_inw_walk.hpp) is listed in the point's cell ("ri_missing"); a
    point outside the bounds is in no leaf box ("ri_bounds"); cells is non-decreasing and ends at
    len(ids) ("ri_cells"); no cell lists more than 64 ids or one id twice, every id < n ("ri_ids")."""
    v = []
    cells = np.asarray(cells, np.int64)
    ids = np.asarray(ids, np.int64)
    d = np.asarray(dim, np.int64)
    nc = int(d[0] * d[1] * d[2])
    if len(cells) != nc + 1 or cells[0] != 0 or (np.diff(cells) < 0).any() or cells[-1] != len(ids):
        return [("ri_cells", f"{len(cells)} offsets for {nc} cells, last {cells[-1] if len(cells) else None}, "
                             f"{len(ids)} ids")]
    if len(ids) and (ids.min() < 0 or ids.max() >= n):
        return [("ri_ids", f"id outside 0..{n - 1}")]
    cnt = np.diff(cells)
    for c in np.flatnonzero(cnt > 64):
        v.append(("ri_ids", f"cell {c} lists {cnt[c]} ids"))
    width = max(1, int(cnt.max()) if nc else 1)
    table = np.full((nc, width), -1, np.int64)
    col = np.arange(len(ids)) - np.repeat(cells[:-1], cnt)
    row = np.repeat(np.arange(nc), cnt)
    table[row, col] = ids
    srt = np.sort(table, axis=1)
    for c in np.flatnonzero(((srt[:, 1:] == srt[:, :-1]) & (srt[:, 1:] >= 0)).any(axis=1)):
        v.append(("ri_ids", f"cell {c} lists an id twice"))
    b = np.ascontiguousarray(wleaf, F32)[:, 0:6]
    p = np.ascontiguousarray(points, F32)
    lo, hi = np.asarray(lo, F32), np.asarray(hi, F32)
    inb = ((p >= lo) & (p <= hi)).all(axis=1)
    cell = ri_cell_of(p, lo, inv, dim)
    bt = np.ascontiguousarray(b.T)  # (6, n)
    for s in range(0, len(p), 2048):
        q, e = p[s:s + 2048], inb[s:s + 2048]
        inside = np.ones((len(q), n), bool)  # brute force: every point against every leaf box
        for a in range(3):
            x = np.ascontiguousarray(q[:, a])[:, None]
            inside &= x >= bt[a][None, :]
            inside &= x <= bt[3 + a][None, :]
        for i, g in zip(*np.nonzero(inside & ~e[:, None])):
            v.append(("ri_bounds", f"point {q[i]} is outside the grid bounds but inside object {g}'s leaf box"))
        listed = np.zeros((len(q), n + 1), bool)
        listed[np.arange(len(q))[:, None], table[cell[s:s + 2048]]] = True  # id -1 lands in column n
        for i, g in zip(*np.nonzero(inside & e[:, None] & ~listed[:, :n])):
            v.append(("ri_missing", f"point {q[i]} (cell {cell[s + i]}) is inside object {g}'s leaf box, "
                                    "which the cell does not list"))
    return v


IOW_CUBOID, IOW_ELLIPSOID = 1, 2


def iow_samples(typ, rec, dirs):
    """World-space surface samples (float64) of one IOW-03 record (24 floats: position, the matrix M
    the shader applies as M * (p - position), column-major, scale): the object is the set of p whose
    M * (p - position) lies on the local surface, so p = position + inverse(M) * local.  Ellipsoid: local
    = scale * unit direction, for `dirs` and the six axis extremes of each world axis; cuboid: its eight
    corners +-scale / 2."""
    r = np.asarray(rec, np.float64)
    pos, M, scale = r[0:3], r[3:12].reshape(3, 3).T, np.abs(r[12:15])
    Minv = np.linalg.inv(M)
    if int(typ) == IOW_ELLIPSOID:
        # the local direction whose world image is extreme along world axis k: scale * row k of Minv
        ext = [s * (Minv[k] * scale) / np.linalg.norm(Minv[k] * scale) for k in range(3) for s in (-1.0, 1.0)]
        u = np.concatenate([dirs, np.eye(3), -np.eye(3), np.array(ext)])
        local = u * scale
    else:
        local = np.array([[sx, sy, sz] for sx in (-.5, .5) for sy in (-.5, .5) for sz in (-.5, .5)]) * scale
    return pos + local @ Minv.T


INW_ELLIPSOID, INW_CUBOID = 1, 2


def inw_samples(record28, ratio, dirs):
    """World-space surface samples (float64) of one INW object (its 28-float GeometryBuff record) at one
    time ratio, as the oracle's intersect_ray places it: centre p - delta (1 - ratio) (p floats 0..2,
    delta 15..17), world point = centre + R local with R's columns floats 3..5, 6..8 and 9..11 (the ray
    goes to object space by R transposed).  Ellipsoid (float 18 = 1): local = scale * unit direction,
    for `dirs`, the +-axes and the six directions whose image is extreme along a world axis; cuboid
    (2): its eight corners +-scale / 2."""
    f = np.asarray(record28, np.float64)
    centre = f[0:3] - f[15:18] * (1.0 - float(ratio))
    Rm = np.stack([f[3:6], f[6:9], f[9:12]], axis=1)
    scale = np.abs(f[12:15])
    if int(f[18] + 0.1) == INW_ELLIPSOID:
        # world_k = sum_c R[k, c] scale_c u_c over unit u: extreme at u along (R[k, c] scale_c)_c
        ext = [s * (Rm[k] * scale) / np.linalg.norm(Rm[k] * scale) for k in range(3) for s in (-1.0, 1.0)]
        u = np.concatenate([dirs, np.eye(3), -np.eye(3), np.array(ext)])
        local = u * scale
    else:
        local = np.array([[sx, sy, sz] for sx in (-.5, .5) for sy in (-.5, .5) for sz in (-.5, .5)]) * scale
    return centre + local @ Rm.T


def unit_dirs(n, seed=5):
    d = np.random.default_rng(seed).normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1)[:, None]


def inw_sample_boxes(geom, ratios, dirs):
    """(n, 6) float64: the box of every object's samples over `ratios` (lo xyz, hi xyz)."""
    out = np.zeros((len(geom), 6))
    for g, rec in enumerate(geom):
        s = np.concatenate([inw_samples(rec, r, dirs) for r in ratios])
        out[g, 0:3], out[g, 3:6] = s.min(axis=0), s.max(axis=0)
    return out


def check_bin_boxes(geom, bins, b, boxes, dirs):
    """boxes (n, 6) float32, the culling boxes of time bin b of `bins`: every surface sample of every
    object at the ratios b / bins, (b + 1/2) / bins and (b + 1) / bins lies inside its box, in exact
    comparison ("bin_box").  Also returns the smallest margin (box face to the nearest sample beyond
    which it lies; negative: a violation)."""
    v, worst = [], np.inf
    bx = np.asarray(boxes, np.float64)
    for g, rec in enumerate(geom):
        s = np.concatenate([inw_samples(rec, (b + h) / bins, dirs) for h in (0.0, 0.5, 1.0)])
        m = min(float((s - bx[g, 0:3]).min()), float((bx[g, 3:6] - s).min()))
        worst = min(worst, m)
        if not ((s >= bx[g, 0:3]).all() and (s <= bx[g, 3:6]).all()):
            v.append(("bin_box", f"bin {b} of {bins}, object {g}: a surface sample lies outside its box by {-m}"))
    return v, worst


def check_iow_cull(types, records, wide, obox, n_dirs=300, seed=3):
    """The IOW-03 culling BVH (wide (N, 32): six float4 of child planes, the links as int bits) and the
    object boxes obox (n, 6): the tree checks of check_wide_tree against obox, and obox[j] contains
    every surface sample of object j (iow_samples) in exact comparison ("obox")."""
    n = len(types)
    wide = np.ascontiguousarray(wide, F32)
    obox = np.asarray(obox, F32)
    v = _tree(wide[:, 0:24].reshape(-1, 6, 4), np.ascontiguousarray(wide[:, 24:28]).view(np.int32), 1, n, obox,
              n_nodes=len(wide))
    rng = np.random.default_rng(seed)
    dirs = rng.normal(size=(n_dirs, 3))
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    ob = obox.astype(np.float64)
    for j in range(n):
        s = iow_samples(types[j], records[j], dirs)
        if not ((s >= ob[j, 0:3]).all() and (s <= ob[j, 3:6]).all()):
            v.append(("obox", f"object {j}: a surface sample lies outside its box"))
    return v


def inw_checks(d, lbvh, n, margin, points=None):
    """name of the check function -> its violations, for a dump in R.inw_host_dump's / R.walk_dump_all's
    keys (cnodes / qnodes where present, the RI grid where built)."""
    out = {
        "leafboxes": check_leafboxes(lbvh, d["leafbox"], n),
        "ranks": check_ranks(lbvh, n, d["rank"], d["dfs_high"]),
        "wide_tree": check_wide_tree(d["wnodes"], 1, n, swept_boxes(d["leafbox"]), n_nodes=d["n_wtree0"],
                                     depth=d["depth"], wbound=d["wbound"], inner=d["leafbox"][:, 0:6]),
    }
    if d.get("cnodes") is not None:
        out["compact"] = check_compact(d["wnodes"], d["cnodes"])
    if d.get("qnodes") is not None:
        out["quantised"] = check_quantised(d["wnodes"], d["qnodes"], margin)
    if d["ri_grid"]:
        if points is None:
            points = ri_points(d["leafbox"], d["ri_lo"], d["ri_hi"], d["ri_inv"], d["ri_dim"])
        out["ri_grid"] = check_ri_grid(d["leafbox"], n, d["ri_cells"], d["ri_ids"], d["ri_lo"], d["ri_hi"],
                                       d["ri_inv"], d["ri_dim"], points)
    return out


def reported(res):
    """check name -> the kinds it reported, for the checks that reported anything."""
    return {k: sorted({kind for kind, _ in v}) for k, v in res.items() if v}
