"""A numpy restatement of the IOW-03 record packer and RI priors (iow_records / iow_priors of
rt_scene_build.hip, which rt_debug_iow_prepare_host exposes and rt_dev_scene_iow03_update_device's kernels
must reproduce byte for byte), and the input classes both are tied to.

hot (n, 20): pos3, type, the rotation's 9 floats, scale3, 1/scale3 (IEEE division), the identity flag (1.0
exactly when the rotation has the bit pattern of glm::mat3(1)).  cold (n, 8): record floats 15..22.
priors (10): the mode of the RIs (record float 20; runs compared by ==, the smallest value among equals),
the ascending distinct bit patterns of {0.0, 1.0} and the RIs when there are at most 8 (zeros past the
count, all zeros otherwise), their count as a float.  RIs that are NaN, or hold -0.0, are outside the
contract and none of the cases has them."""
import numpy as np

IDENTITY_BITS = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], np.float32).view(np.uint32)


def records_ref(types: np.ndarray, rec: np.ndarray):
    types = np.ascontiguousarray(types, np.float32)
    rec = np.ascontiguousarray(rec, np.float32).reshape(-1, 24)
    n = len(types)
    hot, cold = np.zeros((n, 20), np.float32), np.zeros((n, 8), np.float32)
    hot[:, 0:3] = rec[:, 0:3]
    hot[:, 3] = types
    hot[:, 4:13] = rec[:, 3:12]
    hot[:, 13:16] = rec[:, 12:15]
    with np.errstate(all="ignore"):
        hot[:, 16:19] = np.float32(1.0) / rec[:, 12:15]
    hot[:, 19] = (np.ascontiguousarray(rec[:, 3:12]).view(np.uint32) == IDENTITY_BITS).all(axis=1)
    cold[:, 0:8] = rec[:, 15:23]
    return hot, cold


def priors_ref(rec: np.ndarray) -> np.ndarray:
    ri = np.sort(np.ascontiguousarray(rec, np.float32).reshape(-1, 24)[:, 20])
    heads = np.flatnonzero(np.concatenate([[True], ri[1:] != ri[:-1]]))
    lengths = np.diff(np.concatenate([heads, [len(ri)]]))
    out = np.zeros(10, np.float32)
    out[0] = ri[heads[np.argmax(lengths)]]  # (argmax: the first of the longest runs, the smallest value)
    bits = np.unique(np.concatenate([np.array([0.0, 1.0], np.float32), ri]).view(np.uint32))
    vals = np.sort(bits.view(np.float32))
    if len(vals) <= 8:
        out[1:1 + len(vals)] = vals
        out[9] = len(vals)
    return out


def tiled(types, rec, n):
    """n objects: the base records repeated, each whole copy 24 further along x."""
    idx = np.arange(n) % len(types)
    r = rec[idx].copy()
    r[:, 0] += (24.0 * (np.arange(n) // len(types))).astype(np.float32)
    return np.ascontiguousarray(types[idx]), np.ascontiguousarray(r)


def with_ri(types, rec, n, values):
    """n tiled objects whose RIs run through `values` (a list; object j gets values[j % len])."""
    t, r = tiled(types, rec, n)
    r[:, 20] = np.array(values, np.float32)[np.arange(n) % len(values)]
    return t, r


EIGHT = [0.0, 1.0, 1.1, 1.2, 1.3, 1.4, 1.5, 1.6]
ROTATION_ROWS, SCALE_ROWS = 4, 4  # what edge_rows patches, from row 0 on


def edge_rows(types, rec, n):
    """n >= 8 tiled objects whose first rows carry the rotation and scale edge cases: rows 0..3 an exact
    identity, one with -0.0 off the diagonal, one off by an ulp, one with the ulp on an off-diagonal
    zero; rows 4..7 unrotated with a scale of 0, a subnormal, 1e38 and a negative value."""
    t, r = tiled(types, rec, n)
    eye = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], np.float32)
    r[0:8, 3:12] = eye
    r[1, 4] = np.float32(-0.0)
    r[2, 3] = np.nextafter(np.float32(1.0), np.float32(2.0))
    r[3, 8] = np.float32(1e-45)
    r[4, 12], r[5, 13], r[6, 14], r[7, 12] = 0.0, np.float32(1e-40), np.float32(1e38), -2.0
    return t, r


def cases(types, rec, big=1455):
    """(name, types, records) of every input class; the RI classes at a small size and at `big` (more
    than one block of the kernels)."""
    out = [("c2", types.copy(), rec.copy())]
    for n in (1, 2, 3):
        out.append((f"first{n}", types[:n].copy(), rec[:n].copy()))
    for n in (7, big):
        out.append((f"ri_equal_{n}", *with_ri(types, rec, n, [1.5])))
        # 1.3 and 1.5 twice in every six: the smaller wins
        out.append((f"ri_tie_{n}", *with_ri(types, rec, 6 * (n // 6 + 1), [1.5, 1.5, 1.3, 1.3, 2.0, 1.0])))
        out.append((f"ri_eight_{n}", *with_ri(types, rec, max(n, 16), EIGHT)))
        out.append((f"ri_nine_{n}", *with_ri(types, rec, max(n, 18), EIGHT + [1.7])))
    out.append(("edges", *edge_rows(types, rec, 8)))
    return out
