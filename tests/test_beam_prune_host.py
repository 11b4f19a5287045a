"""The beam lists' keep / drop predicate (rt_beam_keep_host: k_inw_beam's own function compiled for
the host, DESIGN.md §5.2 "Pixel beams") against sampled primary rays, no device.

A configuration is a camera, a set of spheres (moving and stationary) and a number of time bins K.
For a few pixel directions the predicate decides every (sphere, bin) from the box the sphere sweeps
in that bin; then rays are sampled as set_beam's comment defines them -- the tip within delta0 of
C0 = co + cd, aimed at F = co + cd * focus, starting one unit behind the tip, a time ratio inside the
bin -- and intersected in float64 with every sphere where it is at that time.  A ray that hits a
sphere its pixel's list dropped fails the test.  So that no case passes for lack of hits or of
drops: at least 1e5 hits over all configurations, and in each one a candidate of the unpruned list
that both prune levels drop."""
import ctypes as C

import numpy as np
import pytest

import rt_amd as R

F32 = np.float32
RAYS = 1500   # per pixel direction and bin
PIXELS = 5


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _spheres(rng, n, pos, D, t_lo, t_hi, lateral, moving):
    """n spheres in a cylinder around the camera axis, central parameters t_lo..t_hi; float32 records
    as the device scene keeps them: (position, RN(1 / scale)), (position - last_position)."""
    a = _unit(np.cross(D, [0.3, 1.0, 0.2]))
    b = np.cross(D, a)
    t = rng.uniform(t_lo, t_hi, n)
    ang, rad = rng.uniform(0, 2 * np.pi, n), lateral * np.sqrt(rng.uniform(0, 1, n))
    p = pos + D * t[:, None] + a * (rad * np.cos(ang))[:, None] + b * (rad * np.sin(ang))[:, None]
    scale = rng.uniform(0.1, 0.4, n).astype(F32)
    delta = rng.uniform(-0.3, 0.3, (n, 3)) * (rng.uniform(0, 1, n) < moving)[:, None]
    rec = np.zeros((n, 8), F32)
    rec[:, :3] = p
    rec[:, 3] = F32(1.0) / scale
    rec[:, 4:7] = delta
    rec[:, 7] = 1.5
    return rec


def _bin_boxes(rec, b, K):
    """The box each sphere sweeps while the time ratio lies in bin b of K, rounded outward."""
    p, d = rec[:, :3].astype(np.float64), rec[:, 4:7].astype(np.float64)
    rho = 1.0 / rec[:, 3].astype(np.float64)
    c0, c1 = p - d * (1.0 - b / K), p - d * (1.0 - (b + 1) / K)
    lo = np.minimum(c0, c1) - rho[:, None] * (1 + 1e-6) - 1e-5
    hi = np.maximum(c0, c1) + rho[:, None] * (1 + 1e-6) + 1e-5
    return np.nextafter(lo.astype(F32), F32(-np.inf)), np.nextafter(hi.astype(F32), F32(np.inf))


def _hits(o, d, ratio, rec):
    """(rays, spheres) bool: the float64 sphere test of t_ellipsoid's rule (the near root, or the far
    one from inside; t > 0) against the sphere where it is at each ray's time."""
    p, dl = rec[:, :3].astype(np.float64), rec[:, 4:7].astype(np.float64)
    rho = 1.0 / rec[:, 3].astype(np.float64)
    c = p[None] - dl[None] * (1.0 - ratio)[:, None, None]
    oc = o[:, None, :] - c
    hb = np.einsum("rsk,rk->rs", oc, d)
    cc = np.einsum("rsk,rsk->rs", oc, oc) - rho[None] ** 2
    det = hb * hb - cc
    sq = np.sqrt(np.maximum(det, 0.0))
    return (det > 0.0) & (-hb + sq > 0.0)


CONFIGS = {
    # name: (camera position, axis, aperture, focus, spheres along the axis t_lo..t_hi, lateral, K, moving share)
    "focus_in_front_K1": ((13.0, 2.0, 3.0), (-1.0, -0.15, -0.25), 0.3, 6.0, 12.0, 60.0, 2.5, 1, 0.5),
    "focus_inside_K2": ((13.0, 2.0, 3.0), (-1.0, -0.15, -0.25), 0.3, 30.0, 8.0, 60.0, 2.5, 2, 0.5),
    "focus_behind_K5": ((0.5, 1.0, -20.0), (0.1, -0.05, 1.0), 0.2, 80.0, 5.0, 50.0, 2.0, 5, 0.7),
    "wide_aperture_near_focus_K2": ((0.0, 0.0, 0.0), (0.2, 0.1, 1.0), 1.0, 10.0, 2.0, 40.0, 3.0, 2, 0.5),
    "wide_aperture_stationary_K1": ((3.0, -2.0, 1.0), (1.0, 0.3, 0.2), 1.0, 10.0, 2.0, 25.0, 2.5, 1, 0.0),
    "straddling_t0_K5": ((1.0, 1.0, 1.0), (0.5, 0.4, -1.0), 0.4, 12.0, -6.0, 20.0, 2.0, 5, 0.6),
    "straddling_t0_stationary_K2": ((-4.0, 0.5, 2.0), (-0.3, 0.2, 1.0), 0.6, 9.0, -5.0, 30.0, 2.0, 2, 0.0),
}
TOTAL_HITS = {}


def _keep(lib, pos, cd, ap, focus, wbound, lo, hi, sph, b, K, prune):
    box = np.concatenate([lo, hi]).astype(F32)
    cand = C.c_int(0)
    rc = lib.rt_beam_keep_host(R.fptr(pos), R.fptr(cd), ap, focus, 1.0, wbound, R.fptr(box),
                               None if sph is None else R.fptr(sph), b, K, prune, C.byref(cand))
    assert rc in (0, 1), rc
    return rc, cand.value


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_no_ray_hits_a_dropped_sphere(name):
    cpos, axis, ap, focus, t_lo, t_hi, lateral, K, moving = CONFIGS[name]
    rng = np.random.default_rng(sorted(CONFIGS).index(name) + 77)
    lib = R.load()
    pos = np.array(cpos, F32)
    D = _unit(np.array(axis, np.float64))
    rec = _spheres(rng, 320, pos.astype(np.float64), D, t_lo, t_hi, lateral, moving)
    boxes = [_bin_boxes(rec, b, K) for b in range(K)]
    wbound = float(max(max(np.abs(lo).max(), np.abs(hi).max()) for lo, hi in boxes)) * 1.01
    n = len(rec)
    hits_total, dropped_candidates, kept = 0, 0, 0
    for _ in range(PIXELS):
        cd = _unit(D + rng.uniform(-0.04, 0.04, 3)).astype(F32)
        cd64, co = cd.astype(np.float64), pos.astype(np.float64)
        c0, foc = co + cd64, co + cd64 * float(F32(focus))
        ea = _unit(np.cross(cd64, [0.0, 1.0, 0.0]))
        eb = np.cross(ea, cd64)
        for b in range(K):
            lo, hi = boxes[b]
            keep1, keep2, cand = np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, bool)
            for g in range(n):
                k0, c = _keep(lib, pos, cd, ap, focus, wbound, lo[g], hi[g], rec[g], b, K, 0)
                k1, _ = _keep(lib, pos, cd, ap, focus, wbound, lo[g], hi[g], rec[g], b, K, 1)
                k2, _ = _keep(lib, pos, cd, ap, focus, wbound, lo[g], hi[g], rec[g], b, K, 2)
                k2box, _ = _keep(lib, pos, cd, ap, focus, wbound, lo[g], hi[g], None, b, K, 2)
                assert k0 == c and k2box == k1           # prune 0 is the candidate test; no record: step 1 only
                assert k2 <= k1 <= k0                    # each level only drops
                cand[g], keep1[g], keep2[g] = c, k1, k2
            # rays of this pixel and bin: the tip in the lens disk around C0, the time inside the bin
            ang, rad = rng.uniform(0, 2 * np.pi, RAYS), 0.5 * ap * np.sqrt(rng.uniform(0, 1, RAYS))
            rad[: RAYS // 4] = 0.5 * ap  # the rim, where the beam is widest
            tip = c0 + ea * (rad * np.cos(ang))[:, None] + eb * (rad * np.sin(ang))[:, None]
            d = _unit(foc - tip)
            ratio = (b + rng.uniform(0, 1, RAYS)) / K
            ratio[:8] = b / K
            h = _hits(tip - d, d, ratio, rec)
            per = h.sum(axis=0)
            bad = np.nonzero((per > 0) & ~keep2)[0]
            assert bad.size == 0, (name, b, "rays hit spheres dropped at prune 2", bad[:5], per[bad[:5]])
            bad = np.nonzero((per > 0) & ~keep1)[0]
            assert bad.size == 0, (name, b, "rays hit spheres dropped at prune 1", bad[:5], per[bad[:5]])
            hits_total += int(per.sum())
            dropped_candidates += int((cand & ~keep1).sum() > 0 and (cand & ~keep2 & keep1).sum() > 0)
            kept += int(keep2.sum())
    TOTAL_HITS[name] = hits_total
    print(f"{name}: hits {hits_total}, spheres kept {kept}, (pixel, bin) pairs with drops at both levels "
          f"{dropped_candidates} of {PIXELS * K}")
    assert dropped_candidates > 0, "no candidate was dropped: the case shows nothing"
    assert hits_total > 0 and kept > 0


def test_enough_hits_over_all_configurations():
    """Runs after the cases above (file order): their hits together."""
    assert set(TOTAL_HITS) == set(CONFIGS), "the configurations did not all run"
    assert sum(TOTAL_HITS.values()) >= 100_000, TOTAL_HITS


def test_argument_errors_and_cameras_without_lists():
    lib = R.load()
    pos, cd = np.zeros(3, F32), _unit(np.array([0.2, 0.1, 1.0])).astype(F32)
    box = np.array([1, 0, 9, 3, 2, 11], F32)  # around the central ray's point at z = 10, (2, 1, 10)
    f = R.fptr
    assert lib.rt_beam_keep_host(f(pos), f(cd), 0.1, 10.0, 1.0, 20.0, f(box), None, 0, 1, 2, None) == 1
    assert lib.rt_beam_keep_host(None, f(cd), 0.1, 10.0, 1.0, 20.0, f(box), None, 0, 1, 2, None) == R.RT_E_ARG
    assert lib.rt_beam_keep_host(f(pos), None, 0.1, 10.0, 1.0, 20.0, f(box), None, 0, 1, 2, None) == R.RT_E_ARG
    assert lib.rt_beam_keep_host(f(pos), f(cd), 0.1, 10.0, 1.0, 20.0, None, None, 0, 1, 2, None) == R.RT_E_ARG
    assert lib.rt_beam_keep_host(f(pos), f(cd), 0.1, 10.0, 1.0, 20.0, f(box), None, 2, 2, 2, None) == R.RT_E_ARG
    assert lib.rt_beam_keep_host(f(pos), f(cd), 0.1, 10.0, 1.0, 20.0, f(box), None, 0, 1, 3, None) == R.RT_E_ARG
    # the focal point too close to the lens for its size: no beam lists for this camera
    assert lib.rt_beam_keep_host(f(pos), f(cd), 1.0, 2.0, 1.0, 20.0, f(box), None, 0, 1, 2, None) == R.RT_E_UNSUPPORTED
    # a box far off the central ray is no candidate at any level
    far = np.array([50, 50, 9, 52, 52, 11], F32)
    cand = C.c_int(7)
    for prune in (0, 1, 2):
        assert lib.rt_beam_keep_host(f(pos), f(cd), 0.1, 10.0, 1.0, 80.0, f(far), None, 0, 1, prune, C.byref(cand)) == 0
        assert cand.value == 0


def test_option_and_path_field_mirrored():
    d = R.default_options()
    assert d.inw_beam_prune == 2 and d.size == C.sizeof(R.RtOptions)
    lib = R.load()
    for bad in (-1, 3):
        o = R.default_options()
        o.inw_beam_prune = bad
        assert lib.rt_options_set(C.byref(o)) == R.RT_E_ARG
    with R.options(inw_beam_prune=0):
        assert R.get_options().inw_beam_prune == 0
    assert R.get_options().inw_beam_prune == 2
    assert dict(R.RtPathInfo._fields_)["beam_prune"] is C.c_int
    tot = (C.c_uint64 * 8)()
    assert lib.rt_debug_beam_lists(None, tot, None, None, None, 0) == R.RT_E_ARG
