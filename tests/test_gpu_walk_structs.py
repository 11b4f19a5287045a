"""The device builds of the culling and bookkeeping structures (rt_build.hip: k_leaves, k_ranks,
k_high, k_sah_level, k_collapse_level, k_ri_bounds, k_ri_cells, k_quantize_wnodes, k_compact_wnodes)
read back with rt_debug_walk_dump and checked directly by tests/walk_struct_ref.py, scene by scene
(tests/walk_struct_cases.py): DESIGN.md §2's "every structure is conservative" for what the kernels
actually read.  Nothing here renders.  tests/test_walk_structs.py shows what the checker reports."""
import numpy as np
import pytest

import rt_amd as R
import walk_struct_cases as K
import walk_struct_ref as W

pytestmark = pytest.mark.gpu


def _scene(c, **opts):
    """A device scene built from the case on the host (rt_dev_scene_inw)."""
    lib = R.load()
    with R.options(**opts):
        s = lib.rt_dev_scene_inw(R.fptr(c.geom), c.n, c.layout, R.fptr(c.nodes), R.fptr(c.lights),
                                 0 if c.lights is None else len(c.lights), 1, -1)
    assert s
    return s


def _update(s, c):
    """rt_dev_scene_inw_update with nodes = NULL: the LBVH and the walk structures built on the device."""
    rc = R.load().rt_dev_scene_inw_update(s, R.fptr(c.geom), c.n, None, R.fptr(c.aabbs), R.fptr(c.lights),
                                          0 if c.lights is None else len(c.lights), None)
    assert rc == 0, rc


def _check_dump(d, c, build):
    """Every INW check on a dump of case c; the leaf-box and rank checks take the dumped LBVH."""
    n = c.n
    assert d["n"] == n and d["build"] == build, d["wide_info"]
    assert d["lbvh"].shape == (2 * n - 1, 8) and d["leafbox"].shape == (n, 8) and d["rank"].shape == (2, n)
    assert len(d["wnodes"]) == len(d["cnodes"]) == len(d["qnodes"]) >= d["n_wtree0"] >= 1
    assert d["wide_info"][0] == d["n_wtree0"] and d["wide_info"][2] == d["depth"]
    # the LBVH's leaves are the objects' boxes
    leaf = W.lbvh_leaves(d["lbvh"], n)
    assert (leaf >= 0).all() and d["lbvh"][leaf, 0:6].tobytes() == c.aabbs.tobytes()
    assert d["ri_grid"] == c.ri_grid, "the RI grid is built / dropped against the expectation"
    res = W.inw_checks(d, d["lbvh"], n, K.qmargin())
    assert ("ri_grid" in res) == bool(c.ri_grid) and "compact" in res and "quantised" in res
    assert W.reported(res) == {}, {k: v[:3] for k, v in res.items() if v}


def _check_bin_tree(d, c, bins, b, **kw):
    """Bin tree b of a dump: its leaf slots hold rt_debug_bin_boxes' boxes (the library's own), and the
    objects themselves: the boxes of walk_struct_ref.inw_samples' surface points at the bin's two end
    ratios (float64, exact comparison; the object moves on a straight line between them)."""
    root = 1 + d["n_wtree0"] + b * d["wbin_stride"]
    v = W.check_wide_tree(d["wnodes"], root, c.n, K.bin_boxes(c.geom, c.n, bins, b), **kw)
    assert v == [], (b, v[:3])
    own = W.inw_sample_boxes(c.geom, (b / bins, (b + 1) / bins), W.unit_dirs(100))
    v = W.check_wide_tree(d["wnodes"], root, c.n, own)
    assert v == [], (b, v[:3])


def _check_ri_equals_host(d, n):
    """The device RI grid against ri_grid_build over the same (dumped) leaf boxes: equal frame, equal
    offsets, equal id sets per cell (the device fill is atomic: no order within a cell)."""
    h = R.inw_host_dump(d["lbvh"], n)
    assert h is not None and h["ri_grid"] == d["ri_grid"]
    assert h["leafbox"].tobytes() == d["leafbox"].tobytes()
    if not d["ri_grid"]:
        return
    assert list(h["ri_dim"]) == list(d["ri_dim"])
    for k in ("ri_lo", "ri_hi", "ri_inv"):
        assert h[k].tobytes() == d[k].tobytes(), k
    assert np.array_equal(h["ri_cells"], d["ri_cells"])
    cells = d["ri_cells"].astype(np.int64)
    key = np.repeat(np.arange(len(cells) - 1), np.diff(cells))  # the cell of each id
    for ids in (h["ri_ids"], d["ri_ids"]):
        assert len(ids) == cells[-1]
    assert np.array_equal(h["ri_ids"][np.lexsort((h["ri_ids"], key))], d["ri_ids"][np.lexsort((d["ri_ids"], key))])


@pytest.mark.parametrize("name", K.NAMES)
def test_device_built_structures_are_conservative(gpu, name):
    """A scene of other geometry updated to the case with nodes = NULL: built on the device (info[7] = 1
    for every scene here, walk_struct_cases.py), then every INW check on the dump, and the device RI
    grid against the host's."""
    c = K.case(name)
    # a scene of other geometry first (the same record layout: it is fixed at creation)
    other = K.case("refset5" if c.layout == 4 else "random5" if name == "grid9" else "grid9")
    lib = R.load()
    s = _scene(other)
    try:
        _update(s, c)
        d = R.walk_dump_all(s)
    finally:
        lib.rt_dev_scene_free(s)
    assert d["wbins"] == 1 and len(d["wnodes"]) == d["n_wtree0"]  # the device builds no bin trees
    _check_dump(d, c, c.build)
    _check_ri_equals_host(d, c.n)


def test_device_build_past_the_level_cap_falls_back_to_the_host(gpu):
    """With the cap lowered to 4 levels the 600-object scene is 'too deep': info[7] = 2, named here in
    advance, and the structures (host-built from the device LBVH, bin trees included) pass the same
    checks."""
    c = K.case("random600")
    lib = R.load()
    s = _scene(K.case("grid9"))
    try:
        assert lib.rt_debug_build_level_cap(4) == 0
        _update(s, c)
        d = R.walk_dump_all(s)
    finally:
        lib.rt_debug_build_level_cap(0)
        lib.rt_dev_scene_free(s)
    _check_dump(d, c, 2)
    assert d["wbins"] == 2 and len(d["wnodes"]) == d["n_wtree0"] + 2 * d["wbin_stride"]
    for b in range(2):
        _check_bin_tree(d, c, 2, b)


@pytest.mark.parametrize("name,bins", [("random600", 2), ("random600", 4), ("random600_at990", 4), ("cornell", 2),
                                       ("mixed250", 2), ("mixed250", 4), ("mixed120_l4", 2), ("mixed120_l4", 4)])
def test_fresh_scene_derived_nodes(gpu, name, bins):
    """A fresh host-built scene dumped from the device: the wide nodes are the host builders' bytes, and
    the compact and quantised nodes (always made by the two device kernels) pass their checks over every
    tree, the time-bin trees included."""
    c = K.case(name)
    lib = R.load()
    s = _scene(c, inw_time_bins=bins)
    try:
        d = R.walk_dump_all(s)
    finally:
        lib.rt_dev_scene_free(s)
    n0, nb, stride, wn = K.time_bins(c, bins)
    assert nb == (bins if c.moving else 1)
    assert (d["n_wtree0"], d["wbins"], d["wbin_stride"]) == (n0, nb, stride if nb > 1 else 0)
    assert d["wnodes"].tobytes() == wn.tobytes() and d["lbvh"].tobytes() == c.nodes.tobytes()
    _check_dump(d, c, 0)
    for b in range(nb if nb > 1 else 0):
        _check_bin_tree(d, c, bins, b, wbound=d["wbound"])
    h = R.inw_host_dump(c.nodes, c.n)
    assert h["rank"].tobytes() == d["rank"].tobytes() and h["dfs_high"] == d["dfs_high"]
    if d["ri_grid"]:
        for k in ("ri_cells", "ri_ids", "ri_lo", "ri_hi", "ri_inv", "ri_dim"):
            assert h[k].tobytes() == d[k].tobytes(), k


def test_updates_leave_no_remnant(gpu):
    """One scene updated to fewer objects, then to more (beyond what its buffers held), then to the
    pile that drops the RI grid and back: every dump refers to the new scene alone (counts, the last
    RI offset, the reachable objects)."""
    lib = R.load()
    s = _scene(K.case("random600"))  # host-built, with time-bin trees
    try:
        for name in ("random257", "random1025", "dups300", "random5", "coplanar400"):
            c = K.case(name)
            _update(s, c)
            d = R.walk_dump_all(s)
            assert d["wbins"] == 1 and d["wbin_stride"] == 0 and len(d["wnodes"]) == d["n_wtree0"], name
            _check_dump(d, c, c.build)
            if c.ri_grid:
                assert d["ri_cells"][-1] == len(d["ri_ids"]) and d["ri_ids"].max() < c.n
            else:
                assert d["ri_cells"] is None and d["wide_info"][4] == 0
    finally:
        lib.rt_dev_scene_free(s)
