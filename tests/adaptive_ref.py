"""The reference of the adaptive-pass tests (rt_render_pass_pixels_async, rt_pass_select_async and the loop
of rt_render_adaptive_inw / rt_render_adaptive_iow03): a plain numpy simulation on the per-sample answers
of tests/pass_ref.py's fixtures -- the per-pixel folds including `even`, the error in the stated operation
order in float32, the active rule, and the list in unit order with its {-1, -1} tail."""
import numpy as np

import pass_ref as PR

# rt_pass_aux and rt_pixel (include/rt_hip.h)
AUX_DTYPE = np.dtype([("even", np.float32, 3), ("count", np.uint32)])
PIXEL_DTYPE = np.dtype([("x", np.int32), ("y", np.int32)])
W, H = PR.W, PR.H


def unit_order(w, h, rect=None):
    """The pixels of the rectangle (x0, y0, tw, th; default the whole w x h frame) in the order of the passes'
    units: 8x8 blocks of the rectangle row-major, pixels row-major inside a block, units past the rectangle's
    edge (or outside the image) left out.  Returns (x, y) int32 arrays."""
    x0, y0, tw, th = rect or (0, 0, w, h)
    xs, ys = [], []
    for by in range((th + 7) // 8):
        for bx in range((tw + 7) // 8):
            for l in range(64):
                rx, ry = bx * 8 + (l & 7), by * 8 + (l >> 3)
                x, y = x0 + rx, y0 + ry
                if rx < tw and ry < th and 0 <= x < w and 0 <= y < h:
                    xs.append(x)
                    ys.append(y)
    return np.array(xs, np.int32), np.array(ys, np.int32)


def error(state, aux):
    """The estimate of every pixel, float32, in the stated order: a = acc * RN(1 / n), e = even * RN(1 / h),
    h = (n + 1) / 2, err = (|a.x - e.x| + |a.y - e.y|) + |a.z - e.z|; +inf for n < 2."""
    n = aux["count"].astype(np.int64)
    ok = n >= 2
    nn, hh = np.where(ok, n, 2), np.where(ok, (n + 1) // 2, 1)
    one = np.float32(1.0)
    inv_n, inv_h = (one / nn.astype(np.float32)).astype(np.float32), (one / hh.astype(np.float32)).astype(np.float32)
    with np.errstate(all="ignore"):
        a = (state["acc"] * inv_n[..., None]).astype(np.float32)
        e = (aux["even"] * inv_h[..., None]).astype(np.float32)
        d = np.abs((a - e).astype(np.float32))
        err = ((d[..., 0] + d[..., 1]).astype(np.float32) + d[..., 2]).astype(np.float32)
    return np.where(ok, err, np.float32(np.inf)).astype(np.float32)


def active(state, aux, tol, min_samples, stop):
    """(active mask, err): active iff n < stop and (n < min_samples or not err <= tol)."""
    err = error(state, aux)
    n = aux["count"].astype(np.int64)
    with np.errstate(invalid="ignore"):
        settled = err <= np.float32(tol)
    return (n < stop) & ((n < min_samples) | ~settled), err


def select(state, aux, tol, min_samples, stop, w, h, rect=None, err_in=None):
    """rt_pass_select_async on flat (h * w) state and aux arrays: (list padded with {-1, -1} to the rectangle's
    pixel count, n_active, err image with the bytes of err_in (default +inf) outside the rectangle)."""
    act, err = active(state, aux, tol, min_samples, stop)
    x, y = unit_order(w, h, rect)
    o = y.astype(np.int64) * w + x
    a = act[o]
    lst = np.full(len(o), -1, np.int32).repeat(2).view(PIXEL_DTYPE)
    n_active = int(a.sum())
    lst["x"][:n_active], lst["y"][:n_active] = x[a], y[a]
    out = np.full(h * w, np.inf, np.float32) if err_in is None else np.array(err_in, np.float32).reshape(-1).copy()
    out[o] = err[o]
    return lst, n_active, out


def fold_even(name, out, k0, k1, even=None):
    """`even` after samples [0, k1) from `even` after [0, k0): acc's fold restricted to the even sample
    indices (INW: sample 0's sqrt(colour) assigned, the later ones added; IOW-03: a sum of rgb from 0.0f)."""
    n = out.shape[0]
    ev = np.zeros((n, 3), np.float32) if k0 == 0 or even is None else np.array(even, np.float32)
    for s in range(k0, k1):
        if s & 1:
            continue
        if name == PR.IOW:
            ev = (ev + out["rgb"][:, s]).astype(np.float32)
        else:
            g = np.sqrt(out["rgb"][:, s]).astype(np.float32)
            ev = g if s == 0 else (ev + g).astype(np.float32)
    return ev


def advance(name, out, state, aux, pixels, ns, stop):
    """One listed pass in place on flat (H * W) state and aux: the pixels `pixels` (flat indices, none twice)
    render samples [count, min(count + ns, stop)).  Pixels are grouped by (count, new count), so every fold
    is pass_ref's own.  Returns {slot: count} of the reference's counters of the samples rendered."""
    ctr = {0: 0, 4: 0, 5: 0}
    pixels = np.asarray(pixels, np.int64)
    c0 = aux["count"][pixels].astype(np.int64)
    c1 = np.minimum(c0 + ns, np.maximum(c0, stop))
    for a, b in sorted(set(zip(c0.tolist(), c1.tolist()))):
        if a == b:
            continue
        m = pixels[(c0 == a) & (c1 == b)]
        state[m] = PR.fold(name, out[m], a, b, state[m])
        aux["even"][m] = fold_even(name, out[m], a, b, aux["even"][m])
        aux["count"][m] = b
        o = out[m][:, a:b]
        for slot, key in ((0, "segments"), (4, "drops"), (5, "nans")):
            ctr[slot] += int(o[key].sum())
    return ctr


def write_image(state, aux, pixels, rgba, depth):
    """What a listed pass writes for `pixels`: acc * RN(1 / count) with alpha 1, and the state's depth."""
    pixels = np.asarray(pixels, np.int64)
    inv = (np.float32(1.0) / aux["count"][pixels].astype(np.float32)).astype(np.float32)
    rgba[pixels, :3] = (state["acc"][pixels] * inv[:, None]).astype(np.float32)
    rgba[pixels, 3] = 1.0
    depth[pixels] = state["depth"][pixels]


def loop(name, batch, tol, min_samples=2, max_rounds=None):
    """The loop of the blocking forms on the fixture `name`: zero the aux buffer, list every pixel, then rounds
    of a listed pass with ns = batch and a select.  Returns one dict per round: state, aux, rgba, depth, err,
    list, n_active and counters (of that round), all copies."""
    out = PR.samples(name)
    stop = PR.spp_of(name)
    n = W * H
    state, aux = np.zeros(n, PR.STATE_DTYPE), np.zeros(n, AUX_DTYPE)
    rgba, depth = np.zeros((n, 4), np.float32), np.zeros(n, np.float32)
    lst, n_active, _ = select(state, aux, -1.0, 0, stop, W, H)
    rounds = []
    while n_active > 0 and (max_rounds is None or len(rounds) < max_rounds):
        px = lst["y"][:n_active].astype(np.int64) * W + lst["x"][:n_active]
        ctr = advance(name, out, state, aux, px, batch, stop)
        write_image(state, aux, px, rgba, depth)
        lst, n_active, err = select(state, aux, tol, min_samples, stop, W, H)
        rounds.append(dict(state=state.copy(), aux=aux.copy(), rgba=rgba.copy(), depth=depth.copy(), err=err,
                           list=lst, n_active=n_active, counters=ctr))
    return rounds


# The settings of the GPU tests: fixture -> (batch, tol).  tests/test_adaptive_ref.py checks that none is
# degenerate (at least 3 distinct final counts, at least 10% of the pixels stop before S, at least 10% go
# past the first batch).
SETTINGS = {"cam_random600": (3, 4.5e-5), "cam_cornell": (2, 0.2), "cam_final": (2, 0.1)}
