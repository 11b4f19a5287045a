"""tests/pass_tiles_ref.py against rt_tile_deal: over the shares of a deal, the slots inside the image cover
every pixel exactly once, and the slots of the ragged right and bottom tiles are flagged as outside."""
import numpy as np
import pytest

import pass_tiles_ref as PT
import rt_amd as R

FRAMES = [(16, 9), (37, 23), (100, 60)]


@pytest.mark.parametrize("n_dev", [1, 3, 8])
@pytest.mark.parametrize("T", [16, 32])
@pytest.mark.parametrize("W,H", FRAMES)
def test_shares_cover_every_pixel_once(W, H, T, n_dev):
    order = R.tile_deal(W, H, T, n_dev)
    assert len(order) == -(-W // T) * -(-H // T)
    seen = np.zeros(W * H, np.int64)
    n_slots = 0
    for share in PT.shares(order, n_dev):
        pixel, inside = PT.slots(share, T, W, H)
        assert pixel.shape == inside.shape == (len(share) * T * T,)
        assert np.all(pixel[~inside] == -1) and np.all(pixel[inside] >= 0) and np.all(pixel[inside] < W * H)
        np.add.at(seen, pixel[inside], 1)
        n_slots += len(pixel)
    assert np.all(seen == 1)
    assert n_slots == len(order) * T * T


def test_slots_outside_the_image_are_flagged():
    # the one 16 x 16 tile of the 16 x 9 frame: rows 9..15 are outside
    pixel, inside = PT.slots([(0, 0)], 16, 16, 9)
    assert inside.reshape(16, 16)[:9].all() and not inside.reshape(16, 16)[9:].any()
    assert np.array_equal(pixel[: 16 * 9], np.arange(16 * 9))
    # 37 x 23, T = 16, tile (2, 1): x = 32..47, y = 16..31 -> 5 columns and 7 rows inside
    pixel, inside = PT.slots([(2, 1)], 16, 37, 23)
    m = inside.reshape(16, 16)
    assert m[:7, :5].all() and m.sum() == 35
    assert pixel.reshape(16, 16)[0, 0] == 16 * 37 + 32 and pixel.reshape(16, 16)[6, 4] == 22 * 37 + 36
    # slot = tile * T * T + iy * T + ix: the second tile's slots follow the first's
    pixel, inside = PT.slots([(0, 0), (1, 0)], 16, 37, 23)
    assert pixel[256 + 3 * 16 + 2] == 3 * 37 + 18 and inside[256 + 3 * 16 + 2]
