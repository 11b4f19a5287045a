"""tests/adaptive_tiles_ref.py against what it is built on, without a device: the slot order of a tile list's
units, the tile loop on the fixtures against adaptive_ref.loop through the slot mapping, and the tile select
of a partition's shares against the rectangle select."""
import numpy as np
import pytest

import adaptive_ref as A
import adaptive_tiles_ref as AT
import pass_ref as PR
import pass_tiles_ref as PT
import rt_amd as R

W, H = PR.W, PR.H


def test_unit_order_of_slots():
    """Unit u of a tile is pixel (l & 7, l >> 3) of 8x8 block u >> 6, the blocks row-major inside the tile."""
    for T in (16, 32, 48):
        o = AT.unit_slots(2, T)
        assert sorted(o.tolist()) == list(range(2 * T * T))          # a permutation of the list's slots
        assert o[:8].tolist() == list(range(8)) and o[8] == T         # a block's rows
        assert o[64] == 8 and o[64 * (T // 8)] == 8 * T               # the next block, the next row of blocks
        assert np.array_equal(o[T * T:], o[:T * T] + T * T)           # tile-major
    # the one-tile list of a frame that the tile covers visits the pixels in the rectangle's unit order
    pixel, inside = PT.slots([(0, 0)], 16, W, H)
    o = AT.unit_slots(1, 16)
    x, y = A.unit_order(W, H)
    assert np.array_equal(pixel[o[inside[o]]], y.astype(np.int64) * W + x)


@pytest.mark.parametrize("name", PR.INW + [PR.IOW])
def test_tile_loop_is_the_rectangle_loop(name):
    batch, tol = A.SETTINGS[name]
    ref = A.loop(name, batch, tol)
    got = AT.loop(name, [(0, 0)], 16, batch, tol)
    assert len(got) == len(ref)
    pixel, inside = PT.slots([(0, 0)], 16, W, H)
    px = pixel[inside]
    for i, (g, r) in enumerate(zip(got, ref)):
        for key in ("state", "aux", "rgba", "depth"):
            assert g[key][inside].tobytes() == r[key][px].tobytes(), (name, i, key)
            assert not g[key][~inside].view(np.uint8).any(), (name, i, key)
        e, want = g["err"][inside], r["err"][px]
        assert np.all((e.view(np.uint32) == want.view(np.uint32)) | (np.isnan(e) & np.isnan(want))), (name, i)
        assert np.all(np.isinf(g["err"][~inside]))
        assert g["n_active"] == r["n_active"] and g["counters"] == r["counters"], (name, i)
        n = g["n_active"]
        lst = r["list"][:n]
        assert np.array_equal(pixel[g["list"][:n].astype(np.int64)], lst["y"].astype(np.int64) * W + lst["x"]), (name, i)
        assert np.all(g["list"][n:W * H] == AT.SLOT_NONE) and np.all(g["list"][W * H:] == AT.SLOT_NONE)


def synthetic(n, seed, stop=8):
    """State and aux of n pixels with every kind of entry: counts 0, 1 (err = +inf), up to stop and past it,
    settled and unsettled pixels, NaN sums."""
    rng = np.random.default_rng(seed)
    state, aux = np.zeros(n, PR.STATE_DTYPE), np.zeros(n, A.AUX_DTYPE)
    aux["count"] = rng.integers(0, stop + 2, n)
    state["acc"] = rng.random((n, 3), np.float32) * aux["count"][:, None].astype(np.float32)
    aux["even"] = (state["acc"] * np.float32(0.5) * (1 + (rng.random((n, 3), np.float32) - 0.5) * 0.2)).astype(np.float32)
    quiet = rng.random(n) < 0.3
    aux["even"][quiet] = (state["acc"][quiet] * np.float32(0.5)).astype(np.float32)
    state["acc"][rng.random(n) < 0.05] = np.nan
    return state, aux


def test_a_partition_selects_the_rectangles_pixels():
    w, h, T, stop = 37, 23, 16, 8
    state, aux = synthetic(w * h, 7, stop)
    tol, min_samples = 0.05, 3
    lst, n_active, err = A.select(state, aux, tol, min_samples, stop, w, h)
    want = set((lst["y"][:n_active].astype(np.int64) * w + lst["x"][:n_active]).tolist())
    assert 0 < n_active < w * h
    order = R.tile_deal(w, h, T, 3)
    got, total = [], 0
    for tiles in PT.shares(order, 3):
        pixel, inside = PT.slots(tiles, T, w, h)
        st, ax = AT.pack(state, tiles, T, w, h), AT.pack(aux, tiles, T, w, h)
        sl, n, e = AT.select(st, ax, tol, min_samples, stop, tiles, T, w, h)
        px = pixel[sl[:n].astype(np.int64)]
        assert (px >= 0).all() and np.all(sl[n:inside.sum()] == AT.SLOT_NONE)
        assert np.array_equal(np.sort(sl[:n]), np.flatnonzero(A.active(st, ax, tol, min_samples, stop)[0] & inside))
        ee, ww = e[inside], err[pixel[inside]]
        assert np.all((ee.view(np.uint32) == ww.view(np.uint32)) | (np.isnan(ee) & np.isnan(ww)))
        got += px.tolist()
        total += int(inside.sum())
    assert total == w * h and len(got) == len(set(got)) == n_active and set(got) == want
