"""The reference of the progressive-pass tests (rt_render_pass_async): plain numpy prefix folds over the
per-sample answers the path-query fixtures already hold -- paths_cam_random600.npz and
paths_cam_cornell.npz (INW, tests/path_ref.py) and path_iow_cam_final.npz (IOW-03,
tests/path_iow_ref.py), every ray a camera ray of a 16 x 9 frame in (y, x, s) order.  A pixel's state
after k samples and the image a pass writes from it; tests/test_pass_ref.py ties k = spp to the
oracle's frames and checks that a fold cut anywhere and continued from the state gives the same bytes."""
import numpy as np

import path_iow_ref as PI
import path_ref as P

# rt_pass_state (include/rt_hip.h), 32 bytes
STATE_DTYPE = np.dtype([("acc", np.float32, 3), ("depth", np.float32), ("ri", np.float32, 4)])
INW = list(P.CAM)        # "cam_random600" (INW-01), "cam_cornell" (INW-04)
IOW = "cam_final"
W, H = P.CAM_W, P.CAM_H
assert (PI.CAM_W, PI.CAM_H) == (W, H)


def spp_of(name: str) -> int:
    return PI.SPP if name == IOW else P.SPP


def samples(name: str):
    """The fixture's per-sample answers as (pixels, spp) records: the frame's own child order on INW."""
    if name == IOW:
        return PI.load_fixture(IOW)["out"].reshape(W * H, PI.SPP)
    fx = P.load_fixture(name)
    return fx.out[P.camera_invert(fx.camera)].reshape(W * H, P.SPP)


def fold(name: str, out, k0: int, k1: int, state=None):
    """The state after samples [0, k1) from the state after [0, k0) (ignored, and may be None, when k0 ==
    0), by the shaders' folds in float32, sample by sample.
    INW: End() -- the first sample's sqrt(colour) assigned, the others added; depth = the depth of sample
    spp / 2 once it has run, else 0; ri stays as it came (0 from a fresh state).
    IOW-03: out_Pixel's sum from 0; depth = 0; ri = the ri_out of the last sample run."""
    n, spp = out.shape
    assert 0 <= k0 <= k1 <= spp
    st = np.zeros(n, STATE_DTYPE)
    if k0 > 0:
        st[:] = state
    acc, depth = st["acc"].copy(), st["depth"].copy()
    for s in range(k0, k1):
        if name == IOW:
            acc = (acc + out["rgb"][:, s]).astype(np.float32)
            st["ri"] = out["ri_out"][:, s]
        else:
            g = np.sqrt(out["rgb"][:, s]).astype(np.float32)
            acc = g if s == 0 else (acc + g).astype(np.float32)
            if s == spp // 2:
                depth = out["depth"][:, s].copy()
    st["acc"], st["depth"] = acc, depth
    return st


def state(name: str, k: int):
    """The state of every pixel of the fixture's frame after samples [0, k), (y, x) order."""
    return fold(name, samples(name), 0, k)


def image(st, k: int):
    """What a pass that ends at k samples writes from the state: rgba = acc * RN(1 / k) with alpha 1 (P, 4),
    and the state's depth (P,)."""
    inv = np.float32(1.0) / np.float32(k)
    rgba = np.ones((len(st), 4), np.float32)
    rgba[:, :3] = (st["acc"] * inv).astype(np.float32)
    return rgba, st["depth"].copy()


def counters(name: str, k0: int, k1: int, pixels=None):
    """The reference's counters of samples [k0, k1) of the frame (or of its pixels `pixels`, a mask in (y, x)
    order): {slot: count} for slots 0 (segments), 4 (dropped pushes), 5 (NaN directions).  (Shadow
    queries, slot 3, are counted per frame only.)"""
    o = samples(name)[:, k0:k1]
    if pixels is not None:
        o = o[pixels]
    return {0: int(o["segments"].sum()), 4: int(o["drops"].sum()), 5: int(o["nans"].sum())}
