"""Adaptive rounds on a device group (rt_render_adaptive_multi_async, rt_group_adaptive_active,
rt_render_adaptive_inw_multi) on the GPU.  A one-device group, as in tests/test_gpu_pass_multi.py: its tiles
still travel through RCCL.  Every equality is a byte equality: after every round the device-0 image, depth and
counts against the single-device loop (rt_render_pass_pixels_async + rt_pass_select_async) on the same scene,
the active count against its n_active, the ray-level counters at the end.  Where a second GPU exists the first
case also runs on devices [0, 1]."""
import ctypes as C

import numpy as np
import pytest

import rt_amd as R
import test_gpu_adaptive as TA
import test_gpu_pass_multi as TM

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = TM.SENTINEL
same, stream, is_iow = TM.same, TM.stream, TM.is_iow
BATCH = {"inw01": 4, "cornell": 2, "iow03": 2}
MIN_SAMPLES = 2


class Frame(TM.Frame):
    """TM.Frame with the W x H sample counts, SENTINEL bytes at first."""

    def __init__(self, p):
        super().__init__(p)
        self.d_count = torch.full((self.n * 4,), SENTINEL, dtype=torch.uint8, device=self.d_rgba.device)

    def count(self):
        return self.d_count.cpu().numpy().view(np.uint32)

    def untouched(self):
        return all(bool((t == SENTINEL).all()) for t in (self.d_rgba, self.d_depth, self.d_count)) and \
            not self.counters().any()


def round_(grp, first, ns, tol, tile, fr, params=None, image=True):
    rc = R.render_adaptive_multi_round(grp.g, grp.scenes, grp.sc.camera, params or grp.sc.params, tile, first, ns, tol,
                                       MIN_SAMPLES, fr.d_rgba if image else None, fr.d_depth if image else None,
                                       fr.d_count, fr.d_ctr, stream())
    torch.cuda.synchronize()
    return rc


def single_device(s, sc, batch, params=None):
    """The single-device loop on the scene handle s: (tol, one dict per round: rgba, depth, count, n_active and
    the counters so far).  tol is the median of the finite err values of its own select after the first round."""
    fr = TA.Frame(s, sc, params)
    assert fr.run_select(-1.0, 0, err=False) == R.RT_OK
    tol, rounds = None, []
    while fr.n_active() > 0:
        assert len(rounds) <= fr.p.spp
        assert fr.run_pass(fr.cap, batch) == R.RT_OK
        if tol is None:
            assert fr.run_select(0.0, MIN_SAMPLES) == R.RT_OK
            e = fr.err()
            tol = float(np.median(e[np.isfinite(e)]))
        assert fr.run_select(tol, MIN_SAMPLES) == R.RT_OK
        rounds.append(dict(rgba=fr.rgba().copy(), depth=fr.depth().copy(), count=fr.aux()["count"].copy(),
                           n_active=fr.n_active(), counters=fr.counters().copy()))
    assert len(rounds) >= 2 and len(np.unique(rounds[-1]["count"])) >= 2   # some pixels stop early
    return tol, rounds


def run_case(name, devices):
    make, tile, _ = TM.CASES[name]
    sc = make()
    slots = TM.IOW_COUNTERS if is_iow(sc) else TM.INW_COUNTERS
    grp = TM.Group(sc, devices)
    try:
        tol, want = single_device(grp.handles[0], sc, BATCH[name])
        fr = Frame(sc.params)
        for i, r in enumerate(want):
            assert round_(grp, i == 0, BATCH[name], tol, tile, fr) == R.RT_OK, i
            what = f"{name} round {i}"
            same(fr.rgba(), r["rgba"], what + ": image")
            same(fr.depth(), r["depth"], what + ": depth")
            same(fr.count(), r["count"], what + ": counts")
            assert R.group_adaptive_active(grp.g) == r["n_active"], what
        assert want[-1]["n_active"] == 0
        for k in slots:
            assert int(fr.counters()[k]) == int(want[-1]["counters"][k]), k
        # one more round finds every list empty: nothing is rendered, the buffers hold the same frame
        assert round_(grp, False, BATCH[name], tol, tile, fr) == R.RT_OK
        same(fr.rgba(), want[-1]["rgba"], f"{name}: a round with empty lists")
        same(fr.count(), want[-1]["count"], f"{name}: its counts")
        for k in slots:
            assert int(fr.counters()[k]) == int(want[-1]["counters"][k]), k
        # a frame whose first round has no image: the later rounds bring every pixel of it
        two = Frame(sc.params)
        assert round_(grp, True, BATCH[name], tol, tile, two, image=False) == R.RT_OK
        assert bool((two.d_rgba == SENTINEL).all()) and bool((two.d_depth == SENTINEL).all())
        same(two.count(), want[0]["count"], f"{name}: counts without an image")
        assert round_(grp, False, BATCH[name], tol, tile, two) == R.RT_OK
        same(two.rgba(), want[1]["rgba"], f"{name}: the second round's image after a round without one")
        same(two.depth(), want[1]["depth"], f"{name}: its depth")
    finally:
        grp.close()


@pytest.mark.parametrize("name", list(TM.CASES))
def test_one_device_group(gpu, name):
    run_case(name, (0,))


def test_two_device_group(gpu):
    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU: no group of more than one device")
    run_case("inw01", (0, 1))


def test_sequence_rules(gpu):
    make, tile, _ = TM.CASES["cornell"]
    sc = make()
    batch = BATCH["cornell"]
    small = R.RtParams.from_buffer_copy(sc.params)
    small.width, small.height = 48, 32
    grp = TM.Group(sc)
    try:
        tol, want = single_device(grp.handles[0], sc, batch)
        assert len(want) >= 3
        fr = Frame(sc.params)
        n = C.c_uint32(77)
        assert R.load().rt_group_adaptive_active(grp.g, C.byref(n)) == R.RT_E_ARG and n.value == 77
        assert round_(grp, False, batch, tol, tile, fr) == R.RT_E_ARG            # no frame was begun
        assert fr.untouched()
        other = R.RtParams.from_buffer_copy(sc.params)
        other.spp = sc.params.spp + 4
        assert round_(grp, True, batch, tol, tile, fr, params=other) == R.RT_E_ARG   # not the scenes' spp
        other.spp, other.show_normal = sc.params.spp, 1
        assert round_(grp, True, batch, tol, tile, fr, params=other) == R.RT_E_UNSUPPORTED
        assert round_(grp, True, 0, tol, tile, fr) == R.RT_OK and fr.untouched()  # ns == 0: nothing launched
        assert round_(grp, False, batch, tol, tile, fr) == R.RT_E_ARG            # ... and no frame begun
        assert round_(grp, True, batch, tol, tile, fr) == R.RT_OK
        same(fr.rgba(), want[0]["rgba"], "first round")
        # a progressive pass may not continue into the adaptive frame
        prog = TM.Frame(sc.params)
        assert grp.pass_(batch, 1, tile, prog) == R.RT_E_ARG
        assert bool((prog.d_rgba == SENTINEL).all())
        # a whole frame between two rounds changes nothing
        whole = TM.Frame(sc.params)
        assert grp.frame(tile, whole) == R.RT_OK
        assert round_(grp, False, batch, tol, tile, fr) == R.RT_OK
        same(fr.rgba(), want[1]["rgba"], "second round after a whole frame")
        same(fr.depth(), want[1]["depth"], "its depth")
        same(fr.count(), want[1]["count"], "its counts")
        assert R.group_adaptive_active(grp.g) == want[1]["n_active"]
        # a progressive pass since the last round: the states are no adaptive frame's any more
        keep = (fr.rgba().copy(), fr.depth().copy(), fr.count().copy(), fr.counters().copy())
        assert grp.pass_(0, 1, tile, prog) == R.RT_OK
        assert round_(grp, False, batch, tol, tile, fr) == R.RT_E_ARG
        for got, was in zip((fr.rgba(), fr.depth(), fr.count(), fr.counters()), keep):
            assert got.tobytes() == was.tobytes()                                # nothing written
        # the deal changed
        assert round_(grp, True, batch, tol, tile, fr) == R.RT_OK
        assert round_(grp, False, batch, tol, tile, Frame(small), params=small) == R.RT_E_ARG
        sm = Frame(small)
        assert round_(grp, True, batch, tol, tile, sm, params=small) == R.RT_OK
        fr2 = Frame(sc.params)
        assert round_(grp, False, batch, tol, tile, fr2) == R.RT_E_ARG and fr2.untouched()
        # ... and a frame begins again at any time
        assert round_(grp, True, batch, tol, tile, fr2) == R.RT_OK
        same(fr2.rgba(), want[0]["rgba"], "a new frame's first round")
        same(fr2.count(), want[0]["count"], "its counts")
    finally:
        grp.close()


def test_blocking_form(gpu):
    make, tile, _ = TM.CASES["cornell"]
    sc = make()
    batch = BATCH["cornell"]
    grp = TM.Group(sc)
    try:
        tol, _ = single_device(grp.handles[0], sc, batch)
    finally:
        grp.close()
    one = R.render_adaptive(sc, batch, tol, MIN_SAMPLES)
    multi = R.render_adaptive_multi(sc, [0], batch, tol, MIN_SAMPLES, tile=tile)
    assert multi["rounds"] == one["rounds"] >= 2
    same(multi["rgba"], one["rgba"], "rt_render_adaptive_inw_multi against rt_render_adaptive_inw")
    same(multi["depth"], one["depth"], "depth")
    same(multi["count"], one["count"], "count")
    assert len(np.unique(one["count"])) >= 2
    for k in ("segments", "shadow_queries", "stack_drops", "nan_drops"):
        assert multi["stats"][k] == one["stats"][k], k
    assert one["stats"]["shadow_queries"] > 0
    capped = R.render_adaptive_multi(sc, [0], batch, tol, MIN_SAMPLES, max_rounds=1, tile=tile)
    assert capped["rounds"] == 1 and np.all(capped["count"] == batch)
