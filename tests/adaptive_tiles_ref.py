"""The reference of the adaptive-pass tests on packed tile lists (rt_render_pass_slots_async,
rt_pass_select_tiles_async): the slot order of a tile list's units and the tile select in plain numpy, built
on tests/adaptive_ref.py (the folds, the error, the active rule) and tests/pass_tiles_ref.py (the slot
mapping).  A packed buffer holds, for every slot inside the image, what the W x H buffer holds for its pixel."""
import numpy as np

import adaptive_ref as A
import pass_ref as PR
import pass_tiles_ref as PT

SLOT_NONE = 0xFFFFFFFF  # RT_SLOT_NONE


def unit_slots(n_tiles: int, T: int):
    """The slots of a list of n_tiles T x T tiles in the order of the tile passes' units: tile-major, 8x8 blocks
    row-major inside a tile, pixels row-major inside a block."""
    per = T // 8
    u = np.arange(n_tiles * T * T, dtype=np.int64)
    t, r = np.divmod(u, T * T)
    b, l = np.divmod(r, 64)
    ix, iy = (b % per) * 8 + (l & 7), (b // per) * 8 + (l >> 3)
    return t * T * T + iy * T + ix


def pack(flat, tiles, T: int, W: int, H: int):
    """The packed buffer of the (W * H, ...) array `flat`: its pixel's record in every slot inside the image,
    zeros in the others."""
    pixel, inside = PT.slots(tiles, T, W, H)
    out = np.zeros((len(pixel),) + flat.shape[1:], flat.dtype)
    out[inside] = flat[pixel[inside]]
    return out


def select(state, aux, tol, min_samples, stop, tiles, T: int, W: int, H: int, slots_in=None, err_in=None):
    """rt_pass_select_tiles_async on packed state and aux: (the slot list -- the active slots in unit order,
    SLOT_NONE up to the number of slots inside the image, the bytes of slots_in (default SLOT_NONE) past that --,
    n_active, the packed err with the bytes of err_in (default +inf) in the slots outside the image)."""
    n = len(np.asarray(tiles).reshape(-1, 2)) * T * T
    _, inside = PT.slots(tiles, T, W, H)
    act, err = A.active(state, aux, tol, min_samples, stop)
    order = unit_slots(n // (T * T), T)
    order = order[inside[order]]
    a = act[order]
    lst = np.full(n, SLOT_NONE, np.uint32) if slots_in is None else np.array(slots_in, np.uint32).reshape(-1).copy()
    n_active = int(a.sum())
    lst[:len(order)] = SLOT_NONE
    lst[:n_active] = order[a]
    out = np.full(n, np.inf, np.float32) if err_in is None else np.array(err_in, np.float32).reshape(-1).copy()
    out[inside] = err[inside]
    return lst, n_active, out


def loop(name, tiles, T: int, batch, tol, min_samples=2, max_rounds=None):
    """adaptive_ref.loop on the packed buffers of the list `tiles` of the fixture `name` (which must cover no
    pixel twice): the aux zeroed, every slot inside the image listed, then rounds of a pass over the listed
    slots with ns = batch and a tile select.  The folds run on the W x H buffers through the slot mapping.
    Returns one dict per round: the packed state, aux, rgba, depth, err, list, n_active and that round's
    counters; the slots outside the image hold zeros (err: +inf)."""
    W, H = PR.W, PR.H
    out = PR.samples(name)
    stop = PR.spp_of(name)
    pixel, inside = PT.slots(tiles, T, W, H)
    n = W * H
    state, aux = np.zeros(n, PR.STATE_DTYPE), np.zeros(n, A.AUX_DTYPE)
    rgba, depth = np.zeros((n, 4), np.float32), np.zeros(n, np.float32)
    packed = lambda: (pack(state, tiles, T, W, H), pack(aux, tiles, T, W, H))
    lst, n_active, _ = select(*packed(), -1.0, 0, stop, tiles, T, W, H)
    rounds = []
    while n_active > 0 and (max_rounds is None or len(rounds) < max_rounds):
        px = pixel[lst[:n_active].astype(np.int64)]
        assert (px >= 0).all()
        ctr = A.advance(name, out, state, aux, px, batch, stop)
        A.write_image(state, aux, px, rgba, depth)
        st, ax = packed()
        lst, n_active, err = select(st, ax, tol, min_samples, stop, tiles, T, W, H)
        rounds.append(dict(state=st, aux=ax, rgba=pack(rgba, tiles, T, W, H), depth=pack(depth, tiles, T, W, H),
                           err=err, list=lst, n_active=n_active, counters=ctr))
    return rounds
