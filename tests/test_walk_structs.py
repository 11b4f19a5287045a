"""DESIGN.md §2 rests every fast path on one statement: a culling or bookkeeping structure may have
any shape because it only rejects work the reference would also reject.  These tests check that
statement on the structures themselves (not through rendered frames) for the host builders, with the
plain checker tests/walk_struct_ref.py, and first show that the checker reports each kind of damage it
is for.  tests/test_gpu_walk_structs.py does the same for the device builds."""
import numpy as np
import pytest

import rt_amd as R
import trace_iow_ref as T
import walk_struct_cases as K
import walk_struct_ref as W

F32 = np.float32


# ------------------------------------------------------------------ derived forms, in numpy
def np_compact(wn):
    return np.concatenate([wn[:, 0:24], wn[:, 36:40]], axis=1).copy()


def _down(x):
    f = F32(x)
    return np.nextafter(f, F32(-np.inf)) if float(f) > x else f


def _up(x):
    f = F32(x)
    return np.nextafter(f, F32(np.inf)) if float(f) < x else f


def np_quantise(wn, m):
    """A straightforward outward quantisation (DESIGN.md §2 "Quantised nodes"), so that the CPU tests
    have a clean quantised form to damage: the checker is not tied to the device kernel's choices."""
    lk, pl = W.links_of(wn), W.planes_of(wn).astype(np.float64)
    q = np.zeros((len(wn), 16), F32)
    u = q.view(np.uint32)
    for w in range(len(wn)):
        live = lk[w] != W.EMPTY
        for a in range(3):
            nlo = pl[w, a][live].min() if live.any() else 0.0
            nhi = pl[w, 3 + a][live].max() if live.any() else 0.0
            o = _down(nlo - m)
            s = _up(max((nhi + m - float(o)) / 255.0, 1e-4))
            while float(o) + 255.0 * float(s) < nhi + m:
                s = np.nextafter(s, F32(np.inf))
            ql = qh = 0
            for k in range(4):
                a_lo, a_hi = 255, 0
                if live[k]:
                    a_lo = min(255, max(0, int(np.floor((pl[w, a, k] - m - float(o)) / float(s)))))
                    while a_lo > 0 and float(o) + a_lo * float(s) > pl[w, a, k] - m:
                        a_lo -= 1
                    a_hi = min(255, max(0, int(np.ceil((pl[w, 3 + a, k] + m - float(o)) / float(s)))))
                    while a_hi < 255 and float(o) + a_hi * float(s) < pl[w, 3 + a, k] + m:
                        a_hi += 1
                ql |= a_lo << (8 * k)
                qh |= a_hi << (8 * k)
            q[w, a], q[w, 3 + a] = o, s
            u[w, 6 + a], u[w, 9 + a] = ql, qh
        u[w, 12:16] = lk[w].view(np.uint32)
    return q


# ------------------------------------------------------------------ the checker catches what it is for
@pytest.fixture(scope="module")
def clean():
    """A clean host-built dump of the 600-object random scene with numpy-derived compact and quantised
    forms, its RI points, and the IOW-03 'rot' set's culling BVH."""
    c = K.case("random600")
    d = R.inw_host_dump(c.nodes, c.n)
    m = K.qmargin()
    d["cnodes"] = np_compact(d["wnodes"])
    d["qnodes"] = np_quantise(d["wnodes"], m)
    pts = W.ri_points(d["leafbox"], d["ri_lo"], d["ri_hi"], d["ri_inv"], d["ri_dim"])
    fx = T.load_fixture("rot")
    iow = R.iow_host_dump(fx["types"], fx["records"], len(fx["types"]))
    assert W.reported(W.inw_checks(d, c.nodes, c.n, m, pts)) == {}
    assert W.check_iow_cull(fx["types"], fx["records"], iow["wide"], iow["obox"]) == []
    return c, d, m, pts, fx, iow


def _copy(d):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in d.items()}


def _leaf_slot(wn):
    lk = W.links_of(wn)
    w, k = np.argwhere((lk <= 0) & (np.arange(len(wn))[:, None] > 0))[7]  # some leaf slot below the root
    return int(w), int(k)


def _rederive(d, m):
    d["cnodes"] = np_compact(d["wnodes"])
    d["qnodes"] = np_quantise(d["wnodes"], m)


def test_checker_reports_a_leaf_plane_one_ulp_inward(clean):
    c, d0, m, pts, _, _ = clean
    for row, toward in ((3, -np.inf), (0, np.inf)):  # a high plane, a low plane (both copies)
        d = _copy(d0)
        w, k = _leaf_slot(d["wnodes"])
        col = 4 * row + k
        d["wnodes"][w, col] = np.nextafter(d["wnodes"][w, col], F32(toward))
        if row < 3:
            d["wnodes"][w, 24 + col] = d["wnodes"][w, col]
        _rederive(d, m)  # the derived forms follow the wide nodes, as in the library
        assert W.reported(W.inw_checks(d, c.nodes, c.n, m, pts)) == {"wide_tree": ["leaf_box"]}


def test_checker_reports_an_object_linked_twice(clean):
    c, d0, m, pts, _, _ = clean
    d = _copy(d0)
    lk = W.links_of(d["wnodes"])
    slots = np.argwhere(lk < 0)
    (w0, k0), (w1, k1) = slots[3], slots[40]
    a, b = -lk[w0, k0], -lk[w1, k1]
    d["wnodes"][w1, 36 + k1] = d["wnodes"][w0, 36 + k0]  # object a twice, object b never
    _rederive(d, m)
    res = W.inw_checks(d, c.nodes, c.n, m, pts)
    assert set(res) - {k for k, v in res.items() if not v} == {"wide_tree"}
    kinds = {kind for kind, _ in res["wide_tree"]}
    assert "reach" in kinds and kinds <= {"reach", "leaf_box", "margin"}
    text = " ".join(msg for kind, msg in res["wide_tree"] if kind == "reach")
    assert f"object {a} reached 2" in text and f"object {b} reached 0" in text


def test_checker_reports_an_id_missing_from_an_ri_cell(clean):
    c, d0, m, pts, _, _ = clean
    d = _copy(d0)
    # a cell that a leaf-box corner falls in needs that object: drop it from there
    g = 17
    corner = d["leafbox"][g:g + 1, 0:3]
    cell = int(W.ri_cell_of(corner, d["ri_lo"], d["ri_inv"], d["ri_dim"])[0])
    b, e = int(d["ri_cells"][cell]), int(d["ri_cells"][cell + 1])
    at = b + int(np.flatnonzero(d["ri_ids"][b:e] == g)[0])
    d["ri_ids"] = np.delete(d["ri_ids"], at)
    d["ri_cells"] = d["ri_cells"].copy()
    d["ri_cells"][cell + 1:] -= 1
    assert W.reported(W.inw_checks(d, c.nodes, c.n, m, pts)) == {"ri_grid": ["ri_missing"]}


def test_checker_reports_swapped_ranks_and_a_low_dfs_high(clean):
    c, d0, m, pts, _, _ = clean
    d = _copy(d0)
    d["rank"][1, [5, 9]] = d["rank"][1, [9, 5]]
    assert W.reported(W.inw_checks(d, c.nodes, c.n, m, pts)) == {"ranks": ["rank"]}
    d = _copy(d0)
    d["dfs_high"] -= 1
    assert W.reported(W.inw_checks(d, c.nodes, c.n, m, pts)) == {"ranks": ["dfs_high"]}


def test_checker_reports_a_quantised_low_byte_plus_one(clean):
    c, d0, m, pts, _, _ = clean
    d = _copy(d0)
    # a slot whose x low plane, one step up, still lies below the wide node's plane but inside the
    # margin: only the margined comparison can see it (steps are below the margin in small nodes)
    org, scl, qlo, _, lk = W.unpack_qnodes(d["qnodes"])
    up = org[:, 0, None].astype(np.float64) + (qlo[:, 0] + 1) * scl[:, 0, None].astype(np.float64)
    lo = W.planes_of(d["wnodes"])[:, 0].astype(np.float64)
    w, k = np.argwhere((lk != W.EMPTY) & (qlo[:, 0] < 255) & (up.astype(F32) <= lo) & (up > lo - m))[0]
    d["qnodes"].view(np.uint32)[w, 6] += np.uint32(1 << (8 * int(k)))
    assert W.reported(W.inw_checks(d, c.nodes, c.n, m, pts)) == {"quantised": ["qplane"]}
    d = _copy(d0)  # and in a large node, where a step is wider than the margin, the decode check sees it too
    w, k = np.argwhere((lk != W.EMPTY) & (qlo[:, 0] < 255) & (up.astype(F32) > lo))[0]
    d["qnodes"].view(np.uint32)[w, 6] += np.uint32(1 << (8 * int(k)))
    assert W.reported(W.inw_checks(d, c.nodes, c.n, m, pts)) == {"quantised": ["qdecode", "qplane"]}


def test_checker_reports_an_altered_compact_row(clean):
    c, d0, m, pts, _, _ = clean
    for col in (4 * 4 + 1, 24 + 2):  # a high plane, a link
        d = _copy(d0)
        d["cnodes"].view(np.uint32)[11, col] ^= 1
        assert W.reported(W.inw_checks(d, c.nodes, c.n, m, pts)) == {"compact": ["compact"]}


def test_checker_reports_an_obox_face_inside_a_sampled_extreme(clean):
    _, _, _, _, fx, iow = clean
    types, rec = fx["types"], fx["records"]
    rng = np.random.default_rng(3)
    dirs = rng.normal(size=(300, 3))
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    for j in (int(np.flatnonzero(types == W.IOW_ELLIPSOID)[0]), int(np.flatnonzero(types == W.IOW_CUBOID)[0])):
        s = W.iow_samples(types[j], rec[j], dirs)
        ob = iow["obox"].copy()
        top = s[:, 1].max()  # the highest sample: put the box's +y face one float below it
        f = F32(top)
        ob[j, 4] = np.nextafter(f, F32(-np.inf)) if float(f) >= top else f
        assert float(ob[j, 4]) < top <= float(np.nextafter(ob[j, 4], F32(np.inf)))  # by less than one ulp
        res = W.check_iow_cull(types, rec, iow["wide"], ob)
        assert [kind for kind, _ in res] == ["obox"] and f"object {j}:" in res[0][1]


# ------------------------------------------------------------------ the host builders
@pytest.mark.parametrize("name", K.NAMES)
def test_host_built_structures_are_conservative(name):
    """inw_wide_build and ri_grid_build over each scene: every check of the checker, and the RI grid
    built exactly where it is expected (dropped only for the pile of identical boxes)."""
    c = K.case(name)
    d = R.inw_host_dump(c.nodes, c.n)
    assert d is not None
    info = R.inw_host_build(c.nodes, c.n)
    assert (info["wide_nodes"], info["dfs_high"], info["wide_depth"]) == (d["n_wtree0"], d["dfs_high"], d["depth"])
    assert d["ri_grid"] == c.ri_grid, "the RI grid is built / dropped against the expectation"
    res = W.inw_checks(d, c.nodes, c.n, K.qmargin())
    assert ("ri_grid" in res) == bool(c.ri_grid)
    assert W.reported(res) == {}, {k: v[:3] for k, v in res.items() if v}


@pytest.mark.parametrize("bins", [2, 4])
@pytest.mark.parametrize("name", ["random600", "random257", "random5", "random600_at990", "mixed250", "mixed120_l4"])
def test_host_built_bin_trees_are_conservative(name, bins):
    """inw_wide_add_bins: the swept tree unchanged in front, then one tree per bin whose leaf slots
    contain rt_debug_bin_boxes' box of the object (test_time_bins.py checks those boxes against the
    moving objects)."""
    c = K.case(name)
    assert c.moving
    d = R.inw_host_dump(c.nodes, c.n)
    n0, nb, stride, wn = K.time_bins(c, bins)
    assert nb == bins and n0 == d["n_wtree0"] and len(wn) == n0 + bins * stride
    assert wn[:n0].tobytes() == d["wnodes"].tobytes()
    assert W.check_wide_tree(wn, 1, c.n, W.swept_boxes(d["leafbox"]), n_nodes=n0, depth=d["depth"]) == []
    for b in range(bins):
        v = W.check_wide_tree(wn, 1 + n0 + b * stride, c.n, K.bin_boxes(c.geom, c.n, bins, b))
        assert v == [], (b, v[:3])
        # ... and the objects themselves at the bin's two end ratios (walk_struct_ref.inw_samples)
        own = W.inw_sample_boxes(c.geom, (b / bins, (b + 1) / bins), W.unit_dirs(100))
        v = W.check_wide_tree(wn, 1 + n0 + b * stride, c.n, own)
        assert v == [], (b, v[:3])
        # padding nodes behind the tree are empty
        assert (W.links_of(wn[n0 + b * stride:n0 + (b + 1) * stride]) != W.EMPTY).any(axis=1).sum() <= stride


@pytest.mark.parametrize("name", ["final", "rot", "touch"])
def test_iow_culling_bvh_is_conservative(name):
    """iow_cull_build over the final scene, the rotated set and the cuboid set of the ray-query
    fixtures: the tree against the object boxes, the object boxes against the objects."""
    fx = T.load_fixture(name)
    types, rec = fx["types"], fx["records"]
    d = R.iow_host_dump(types, rec, len(types))
    assert d is not None and len(d["wide"]) == R.iow_host_build(types, rec, len(types))["wide_nodes"]
    v = W.check_iow_cull(types, rec, d["wide"], d["obox"])
    assert v == [], v[:3]


def test_dump_hooks_validate_arguments():
    lib = R.load()
    c = K.case("grid9")
    assert lib.rt_debug_inw_host_dump(None, 9, None, None, None, None, None, None, None, None) == R.RT_E_ARG
    assert lib.rt_debug_iow_host_dump(None, None, 0, None, None, None) == R.RT_E_ARG
    assert lib.rt_debug_walk_dump(None, 0, None, 0, None) == R.RT_E_ARG
    assert R.inw_host_dump(c.nodes[:1], 1) is None  # one object: no wide walk
    bad = c.nodes.copy()
    bad[bad[:, 6] <= 0.1, 6] = -50.0  # leaves naming an object that does not exist
    assert R.inw_host_dump(bad, c.n) is None
