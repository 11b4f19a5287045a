"""The slot mapping of a packed tile list (rt_render_tiles_async, rt_render_pass_tiles_async) in plain
numpy: slot = tile * T * T + iy * T + ix holds pixel (tx * T + ix, ty * T + iy) when that pixel is inside
the W x H image.  The progressive-pass tests on tile lists and device groups read everything else -- the
states, the images, the counters -- from tests/pass_ref.py through this mapping."""
import numpy as np


def slots(tiles, T: int, W: int, H: int):
    """For the (tx, ty) pairs `tiles`: (pixel, inside), both (len(tiles) * T * T,) -- the pixel index
    y * W + x of every slot (-1 outside the image) and whether the slot is inside the image."""
    t = np.asarray(tiles, np.int64).reshape(-1, 2)
    iy, ix = np.divmod(np.arange(T * T, dtype=np.int64), T)
    x = (t[:, 0, None] * T + ix[None, :]).reshape(-1)
    y = (t[:, 1, None] * T + iy[None, :]).reshape(-1)
    inside = (x < W) & (y < H)
    return np.where(inside, y * W + x, -1), inside


def shares(order, n_dev: int):
    """The deal order's shares: entry k of `order` ((tx, ty) pairs) goes to device k % n_dev."""
    o = np.asarray(order, np.int32).reshape(-1, 2)
    return [np.ascontiguousarray(o[r::n_dev]) for r in range(n_dev)]
