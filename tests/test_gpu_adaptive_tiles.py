"""Adaptive sample passes over packed tile lists (rt_render_pass_slots_async, rt_pass_select_tiles_async) on
the GPU.  Every equality is a byte equality (an err that is a NaN on both sides counts as equal).  A slot
inside the image is its pixel under rt_render_pass_pixels_async + rt_pass_select_async: the fixture frames
round for round against tests/adaptive_tiles_ref.py, the ragged frame against the single-device pair of the
same scene read through the slot mapping of tests/pass_tiles_ref.py.  Slots outside the image and unlisted
slots keep every byte."""
import numpy as np
import pytest

import adaptive_ref as A
import adaptive_tiles_ref as AT
import pass_ref as PR
import pass_tiles_ref as PT
import rt_amd as R
import test_gpu_adaptive as TA
import test_gpu_pass_tiles as TT
import test_gpu_passes as TP

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = TP.SENTINEL
SENT32 = 0xCDCDCDCD
W, H = PR.W, PR.H
NAMES = PR.INW + [PR.IOW]
same, same_state, filled, params_of, scene_of = TP.same, TP.same_state, TP.filled, TP.params_of, TP.scene_of
same_err, same_aux, stream = TA.same_err, TA.same_aux, TA.stream
cached = TT.cached


class TileFrame:
    """The packed buffers of one list's adaptive frame: state, image, err, list and count SENTINEL bytes at
    first, the aux zeroed in the slots inside the image and SENTINEL outside (everywhere with aux_sentinel),
    the counters 0.  The list has four entries more than the list has slots, which must stay SENTINEL."""

    def __init__(self, s, sc, tiles, T, params=None, aux_sentinel=False):
        self.s, self.sc, self.T, self.p = s, sc, T, params or sc.params
        self.tiles = np.ascontiguousarray(tiles, np.int32).reshape(-1, 2)
        self.n_tiles = len(self.tiles)
        self.n = self.n_tiles * T * T
        self.pixel, self.inside = PT.slots(self.tiles, T, self.p.width, self.p.height)
        self.n_inside = int(self.inside.sum())
        dev = torch.device("cuda")
        self.d_tiles = torch.from_numpy(self.tiles.copy()).to(dev)
        self.d_state, self.d_aux = filled(self.n * 32), filled(self.n * 16)
        self.d_rgba, self.d_depth, self.d_err = filled(self.n * 16), filled(self.n * 4), filled(self.n * 4)
        self.d_slots, self.d_n = filled((self.n + 4) * 4), filled(16)
        self.d_ctr = torch.zeros(6, dtype=torch.int64, device=dev)
        if not aux_sentinel:
            aux = self.aux().copy()
            aux[self.inside] = np.zeros(1, R.PASS_AUX_DTYPE)
            self.set_aux(aux)

    def _put(self, t, a):
        b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        t[: len(b)] = torch.from_numpy(b.copy()).to(t.device)

    def set_slots(self, slots):
        a = np.asarray(slots, np.uint32)
        assert len(a) <= self.n + 4
        self._put(self.d_slots, a)
        return len(a)

    def set_aux(self, aux):
        self._put(self.d_aux, aux)

    def set_state(self, st):
        self._put(self.d_state, st)

    def pass_call(self, n_slots, ns, params=None, **kw):
        b = dict(d_tiles=self.d_tiles, n_tiles=self.n_tiles, T=self.T, d_slots=self.d_slots, d_state=self.d_state,
                 d_aux=self.d_aux, d_out=self.d_rgba, d_depth=self.d_depth, d_counters=self.d_ctr)
        b.update(kw)
        return R.pass_slots(self.s, self.sc.camera, params or self.p, b["d_tiles"], b["n_tiles"], b["T"], b["d_slots"],
                            n_slots, ns, b["d_state"], b["d_aux"], b["d_out"], b["d_depth"], b["d_counters"], stream())

    def select_call(self, tol, min_samples, params=None, err=True, **kw):
        b = dict(d_tiles=self.d_tiles, n_tiles=self.n_tiles, T=self.T, d_state=self.d_state, d_aux=self.d_aux,
                 d_slots=self.d_slots, d_n_active=self.d_n)
        b.update(kw)
        return R.pass_select_tiles(self.s, params or self.p, b["d_tiles"], b["n_tiles"], b["T"], b["d_state"],
                                   b["d_aux"], tol, min_samples, b["d_slots"], b["d_n_active"],
                                   self.d_err if err else None, stream())

    def run_pass(self, n_slots, ns, **kw):
        rc = self.pass_call(n_slots, ns, **kw)
        torch.cuda.synchronize()
        return rc

    def run_select(self, tol, min_samples, **kw):
        rc = self.select_call(tol, min_samples, **kw)
        torch.cuda.synchronize()
        return rc

    def state(self):
        return self.d_state.cpu().numpy()[: self.n * 32].view(R.PASS_STATE_DTYPE)

    def aux(self):
        return self.d_aux.cpu().numpy()[: self.n * 16].view(R.PASS_AUX_DTYPE)

    def rgba(self):
        return self.d_rgba.cpu().numpy()[: self.n * 16].view(np.float32).reshape(self.n, 4)

    def depth(self):
        return self.d_depth.cpu().numpy()[: self.n * 4].view(np.float32)

    def err(self):
        return self.d_err.cpu().numpy()[: self.n * 4].view(np.float32)

    def slots(self):
        """(the list's n entries, the four guard entries)"""
        a = self.d_slots.cpu().numpy()[: (self.n + 4) * 4].view(np.uint32)
        return a[: self.n], a[self.n:]

    def n_active(self):
        return int(self.d_n.cpu().numpy()[:4].view(np.uint32)[0])

    def counters(self):
        return self.d_ctr.cpu().numpy()

    def check(self, want, what, listed=None):
        """The slots inside the image (of them those in the mask `listed`, default all) against per-pixel
        references: want = dict of (W * H,) state, aux, rgba, depth and, optionally, err.  Every other slot holds
        SENTINEL bytes."""
        m = self.inside if listed is None else (self.inside & listed)
        px = self.pixel[m]
        iow = TT.is_iow(self.sc)
        st, aux, rgba, depth = self.state(), self.aux(), self.rgba(), self.depth()
        same_state(st[m], want["state"][px], iow, what + ": state")
        same_aux(aux[m], want["aux"][px], what + ": aux")
        same(rgba[m], want["rgba"][px], what + ": image")
        same(depth[m], want["depth"][px], what + ": depth")
        if "err" in want:
            same_err(self.err()[self.inside], want["err"][self.pixel[self.inside]], what + ": err")
            assert np.all(self.err()[~self.inside].view(np.uint32) == SENT32), what + ": err outside the image"
        for a, k in ((st, "state"), (aux, "aux"), (rgba, "image"), (depth, "depth")):
            assert np.all(a[~m].view(np.uint8) == SENTINEL), f"{what}: {k} of a slot that is not the pass's was written"

    def check_list(self, active, what):
        """The list after a select: the slots whose pixel is in the (W * H,) mask `active`, in unit order, then
        RT_SLOT_NONE up to the number of slots inside the image, then the bytes it had."""
        order = AT.unit_slots(self.n_tiles, self.T)
        order = order[self.inside[order]]
        want = order[active[self.pixel[order]]]
        got, guard = self.slots()
        assert self.n_active() == len(want), what
        same(got[: len(want)], want.astype(np.uint32), what + ": list")
        assert np.all(got[len(want): self.n_inside] == R.SLOT_NONE), what + ": padding"
        assert np.all(got[self.n_inside:] == SENT32) and np.all(guard == SENT32), what + ": past the slots inside"

    def loop(self, batch, tol, min_samples=2, after=None):
        """The blocking forms' loop on these buffers: every pass is launched with the list's full capacity right
        behind the select, with nothing read back in between; after(round index) runs after each round."""
        assert self.run_select(-1.0, 0, err=False) == R.RT_OK
        rounds = 0
        while self.n_active() > 0:
            assert rounds <= self.p.spp
            assert self.pass_call(self.n, batch) == R.RT_OK
            assert self.run_select(tol, min_samples) == R.RT_OK
            if after:
                after(rounds)
            rounds += 1
        return rounds


# ------------------------------------------------------------- the fixture frames: one tile, rows 9..15 outside
@pytest.mark.parametrize("name", NAMES)
def test_fixture_frames(gpu, name):
    batch, tol = A.SETTINGS[name]
    ref = AT.loop(name, [(0, 0)], 16, batch, tol)
    sc = scene_of(name)
    iow = name == PR.IOW
    s = R.dev_scene(sc)
    try:
        fr = TileFrame(s, sc, [(0, 0)], 16)
        m = fr.inside
        assert m.sum() == W * H and (~m).sum() == 16 * 7
        total = {0: 0, 4: 0, 5: 0}

        def after(i):
            r, what = ref[i], f"{name} round {i}"
            same_state(fr.state()[m], r["state"][m], iow, what)
            same_aux(fr.aux()[m], r["aux"][m], what)
            same(fr.rgba()[m], r["rgba"][m], what + " rgba")
            same(fr.depth()[m], r["depth"][m], what + " depth")
            same_err(fr.err()[m], r["err"][m], what + " err")
            for a in (fr.state(), fr.aux(), fr.rgba(), fr.depth(), fr.err()):
                assert np.all(a[~m].view(np.uint8) == SENTINEL), what + ": a slot outside the image was written"
            got, guard = fr.slots()
            assert fr.n_active() == r["n_active"], what
            same(got[: W * H], r["list"][: W * H], what + " list")
            assert np.all(got[W * H:] == SENT32) and np.all(guard == SENT32), what
            for k, v in r["counters"].items():
                total[k] += v
                assert int(fr.counters()[k]) == total[k], (what, k)

        assert fr.loop(batch, tol, after=after) == len(ref)
        if iow:
            assert int(fr.counters()[3]) == 0
    finally:
        R.load().rt_dev_scene_free(s)


# ------------------------------------------------------------- the ragged frame
RW, RH, SPP, BATCH = TT.RW, TT.RH, 8, 3


def odd_scene(family):
    return TT.ODD[family](RW, RH, SPP)


def rect_rounds(s, sc):
    """The single-device loop (rt_render_pass_pixels_async + rt_pass_select_async) on the whole 37 x 23 frame,
    batch 3: per round the (W * H,) state, aux, rgba, depth, err, the active mask and the counters so far.  tol
    is the median of the finite err values of its own select after the first round."""
    fr = TA.Frame(s, sc)
    n = RW * RH
    assert fr.run_select(-1.0, 0, err=False) == R.RT_OK
    tol, rounds = None, []
    while fr.n_active() > 0:
        assert len(rounds) <= SPP
        assert fr.run_pass(fr.cap, BATCH) == R.RT_OK
        if tol is None:
            assert fr.run_select(0.0, 2) == R.RT_OK
            e = fr.err()
            tol = float(np.median(e[np.isfinite(e)]))
        assert fr.run_select(tol, 2) == R.RT_OK
        lst = fr.list()[0][: fr.n_active()]
        active = np.zeros(n, bool)
        active[lst["y"].astype(np.int64) * RW + lst["x"]] = True
        rounds.append(dict(state=fr.state().copy(), aux=fr.aux().copy(), rgba=fr.rgba().copy(), depth=fr.depth().copy(),
                           err=fr.err().copy(), active=active, counters=fr.counters().copy()))
    count = rounds[-1]["aux"]["count"]
    print("tol", tol, "rounds", len(rounds), "final counts", dict(zip(*np.unique(count, return_counts=True))))
    # not degenerate: three or more final counts, a tenth of the pixels stop early, a tenth go past the first batch
    assert len(np.unique(count)) >= 3 and (count < SPP).mean() >= 0.1 and (count > BATCH).mean() >= 0.1
    return tol, rounds


def reference(family, s, sc):
    return cached(("adaptive rect", family), lambda: rect_rounds(s, sc))


def ragged_lists():
    lists = dict(TT.ragged_lists())
    lists["one32"] = ([(0, 0)], 32)
    lists["one48"] = ([(0, 0)], 48)
    del lists["full32"]
    return lists


def run_list(s, sc, tol, ref, tiles, T, what):
    """The loop on one list against the reference rounds; the frame after its last round."""
    fr = TileFrame(s, sc, tiles, T)
    everything = np.ones(RW * RH, bool)
    assert fr.run_select(-1.0, 0, err=False) == R.RT_OK
    fr.check_list(everything, what + ": every slot listed")
    for i, r in enumerate(ref):
        assert fr.pass_call(fr.n, BATCH) == R.RT_OK     # the full capacity, no read-back
        assert fr.run_select(tol, 2) == R.RT_OK
        fr.check(r, f"{what} round {i}")
        fr.check_list(r["active"], f"{what} round {i}")
    assert fr.n_active() == 0
    return fr


@pytest.mark.parametrize("which", ["full16", "share1of3", "two16", "one32", "one48"])
@pytest.mark.parametrize("family", list(TT.ODD))
def test_ragged_frame(gpu, family, which):
    sc = odd_scene(family)
    tiles, T = ragged_lists()[which]
    s = R.dev_scene(sc)
    try:
        tol, ref = reference(family, s, sc)
        fr = run_list(s, sc, tol, ref, tiles, T, f"{family} {which}")
        assert (~fr.inside).any()  # every list has slots outside the image
    finally:
        R.load().rt_dev_scene_free(s)


@pytest.mark.parametrize("family", list(TT.ODD))
def test_partition_counters(gpu, family):
    """The counters summed over the three shares of a 3-device deal and all rounds are the single-device loop's."""
    sc = odd_scene(family)
    s = R.dev_scene(sc)
    try:
        tol, ref = reference(family, s, sc)
        total = np.zeros(6, np.int64)
        for r, share in enumerate(PT.shares(R.tile_deal(RW, RH, 16, 3), 3)):
            total += run_list(s, sc, tol, ref, share, 16, f"{family} share {r}").counters()
        for k in TT.counter_slots(sc):
            assert int(total[k]) == int(ref[-1]["counters"][k]), k
    finally:
        R.load().rt_dev_scene_free(s)


# ------------------------------------------------------------- the listed pass alone
@pytest.mark.parametrize("family", list(TT.ODD))
def test_hand_made_list(gpu, family):
    """Every third slot inside the image in a shuffled order, with RT_SLOT_NONE entries, entries at and past
    n_tiles * T * T and slots outside the image among them: the listed slots hold what
    rt_render_pass_pixels_async leaves for their pixels, everything else keeps its SENTINEL bytes."""
    sc = odd_scene(family)
    tiles, T = ragged_lists()["full16"]
    s = R.dev_scene(sc)
    try:
        fr = TileFrame(s, sc, tiles, T, aux_sentinel=True)
        rng = np.random.default_rng(5)
        mine = rng.permutation(np.flatnonzero(fr.inside)[::3])
        listed = np.zeros(fr.n, bool)
        listed[mine] = True
        aux = fr.aux().copy()
        aux[listed] = np.zeros(1, R.PASS_AUX_DTYPE)
        fr.set_aux(aux)
        outside = np.flatnonzero(~fr.inside)
        lst = mine.tolist()
        for at, bad in ((0, R.SLOT_NONE), (7, fr.n), (20, int(outside[0])), (len(lst), R.SLOT_NONE), (3, fr.n + 12345),
                        (9, int(outside[-1])), (40, 0x80000000)):
            lst.insert(at, bad)
        n_list = fr.set_slots(lst)
        one = TA.Frame(s, sc, aux_sentinel=True)     # the single-device pass over the same pixels
        px = fr.pixel[mine]
        a1 = one.aux().copy()
        a1[px] = np.zeros(1, R.PASS_AUX_DTYPE)
        one.set_aux(a1)
        n_px = one.set_list(px % RW, px // RW)
        for ns in (3, 2, SPP, 2):   # the last one finds nothing left: only the image is rewritten
            if ns == 2 and fr.aux()["count"][mine[0]] == SPP:
                fr.d_rgba.fill_(SENTINEL)
                fr.d_depth.fill_(SENTINEL)
                one.d_rgba.fill_(SENTINEL)
                one.d_depth.fill_(SENTINEL)
            assert fr.run_pass(n_list, ns) == R.RT_OK and one.run_pass(n_px, ns) == R.RT_OK
            want = dict(state=one.state(), aux=one.aux(), rgba=one.rgba(), depth=one.depth())
            fr.check(want, f"{family} hand-made + {ns}", listed)
            for k in TT.counter_slots(sc):
                assert int(fr.counters()[k]) == int(one.counters()[k]), (ns, k)
        assert np.all(fr.aux()["count"][mine] == SPP)
    finally:
        R.load().rt_dev_scene_free(s)


class Unpacked:
    """A one-tile TileFrame of a 16 x 9 fixture frame read as the W x H buffers test_gpu_adaptive checks."""

    def __init__(self, fr):
        self.fr = fr

    def _flat(self, a):
        out = np.zeros((W * H,) + a.shape[1:], a.dtype)
        out[self.fr.pixel[self.fr.inside]] = a[self.fr.inside]
        return out

    def state(self):
        return self._flat(self.fr.state())

    def aux(self):
        return self._flat(self.fr.aux())

    def rgba(self):
        return self._flat(self.fr.rgba())

    def depth(self):
        return self._flat(self.fr.depth())


@pytest.mark.parametrize("mode", ["plain", "chunks", "one_block"])
@pytest.mark.parametrize("name,a,b", TA.MIXED, ids=lambda v: str(v))
def test_start_counts_differ_inside_a_wave(gpu, name, a, b, mode):
    """test_gpu_adaptive's case on the one-tile list: a samples on the even pixels' slots, b on the odd ones',
    then one pass of 5 over all slots in unit order.  chunks: the INW workspace holds 2 samples of an entry;
    one_block: one 256-lane block serves the list."""
    sc = scene_of(name)
    spp = PR.spp_of(name)
    lib = R.load()
    s = R.dev_scene(sc)
    prev_chunk = lib.rt_debug_adaptive_chunk(2 if mode == "chunks" else 0)
    prev_blocks = lib.rt_debug_pass_max_blocks(1 if mode == "one_block" else 0)
    try:
        fr = TileFrame(s, sc, [(0, 0)], 16)
        order = AT.unit_slots(1, 16)
        order = order[fr.inside[order]]
        count = np.zeros(W * H, np.int64)
        for parity, ns in ((0, a), (1, b)):
            sel = order[fr.pixel[order] % 2 == parity]
            assert fr.run_pass(fr.set_slots(sel), ns) == R.RT_OK
            count[fr.pixel[sel]] = ns
        assert fr.run_pass(fr.set_slots(order), 5) == R.RT_OK
        count = np.minimum(count + 5, spp)
        TA.check_pixels(Unpacked(fr), name, count, np.ones(W * H, bool), f"{name} {a}/{b} + 5 ({mode})")
        for arr in (fr.state(), fr.aux(), fr.rgba(), fr.depth()):
            assert np.all(arr[~fr.inside].view(np.uint8) == SENTINEL)
        total = {0: 0, 4: 0, 5: 0}
        for k in np.unique(count):
            for slot, v in PR.counters(name, 0, int(k), count == k).items():
                total[slot] += v
        assert all(int(fr.counters()[slot]) == v for slot, v in total.items())
    finally:
        lib.rt_debug_adaptive_chunk(prev_chunk)
        lib.rt_debug_pass_max_blocks(prev_blocks)
        lib.rt_dev_scene_free(s)


# ------------------------------------------------------------- the select kernels alone
def select_lists():
    lists = {k: (tiles, T, RW, RH) for k, (tiles, T) in ragged_lists().items()}
    # 272 tiles of 16 x 16: 272 blocks of units, so the scan's second round starts from the first one's totals
    lists["272tiles"] = ([(x, y) for y in range(16) for x in range(17)], 16, 272, 256)
    return lists


@pytest.mark.parametrize("case", ["full16", "share1of3", "two16", "one32", "one48", "272tiles"])
@pytest.mark.parametrize("family", ["inw", "iow"])
def test_select_alone(gpu, family, case):
    """rt_pass_select_tiles_async on buffers from numpy (NaN, infinities and n < 2 among them), no rendering: list,
    padding, count and err against adaptive_tiles_ref; the slots outside the image keep their err bytes, and the
    list keeps its bytes past the number of slots inside the image."""
    tiles, T, w, h = select_lists()[case]
    name = PR.IOW if family == "iow" else "cam_random600"
    sc = scene_of(name)
    stop = PR.spp_of(name)
    p = params_of(sc, width=w, height=h)
    s = R.dev_scene(sc)
    try:
        fr = TileFrame(s, sc, tiles, T, p)
        st, aux = TA.synthetic(fr.n, stop, np.random.default_rng(len(case) + T), "mixed")
        fr.set_state(st)
        fr.set_aux(aux)
        sent = TP.sentinel_array
        for tol, min_samples in ((0.05, 3), (-1.0, 0)):
            fr.d_slots.fill_(SENTINEL)
            fr.d_n.fill_(SENTINEL)
            assert fr.run_select(tol, min_samples) == R.RT_OK
            lst, n_active, err = AT.select(st, aux, tol, min_samples, stop, tiles, T, w, h,
                                           slots_in=sent(np.uint32, (fr.n,)), err_in=sent(np.float32, (fr.n,)))
            got, guard = fr.slots()
            assert fr.n_active() == n_active and 0 < n_active <= fr.n_inside
            same(got, lst, f"{case}: list")
            assert np.all(guard == SENT32)
            same_err(fr.err(), err, f"{case}: err")
            same(fr.state(), st, f"{case}: the state is only read")
            same(fr.aux(), aux, f"{case}: the aux is only read")
        fr.d_n.fill_(SENTINEL)
        assert fr.run_select(-1.0, 0, err=False) == R.RT_OK   # without an err image
        assert fr.n_active() == n_active
        same(fr.slots()[0], lst, f"{case}: list without err")
    finally:
        R.load().rt_dev_scene_free(s)


# ------------------------------------------------------------- options, errors, resources
@pytest.mark.parametrize("family,option,value,tiles", [("inw01", "inw_wide_walk", 0, None),
                                                        ("iow03", "iow_linear", 1, [(2, 1)])])
def test_options_do_not_change_results(gpu, family, option, value, tiles):
    """The reference comes from a scene with the default options.  (The linear loop tests every object for every
    ray: the tile (2, 1), with 35 pixels inside the image, keeps it short.)"""
    sc = odd_scene(family)
    s = R.dev_scene(sc)
    try:
        tol, ref = reference(family, s, sc)
    finally:
        R.load().rt_dev_scene_free(s)
    with R.options(**{option: value}):
        s = R.dev_scene(sc)  # a scene keeps the options it was created with
    try:
        run_list(s, sc, tol, ref, tiles or R.tile_deal(RW, RH, 16, 3), 16, f"{family} {option}={value}")
    finally:
        R.load().rt_dev_scene_free(s)


@pytest.mark.parametrize("family", list(TT.ODD))
def test_errors_on_a_device(gpu, family):
    sc = odd_scene(family)
    s = R.dev_scene(sc)
    try:
        fr = TileFrame(s, sc, [(0, 0), (2, 1)], 16, aux_sentinel=True)
        order = AT.unit_slots(2, 16)
        n_list = fr.set_slots(order[fr.inside[order]])
        listed = fr.d_slots.clone()

        def untouched(rc, want):
            torch.cuda.synchronize()
            assert rc == want
            for t in (fr.d_state, fr.d_aux, fr.d_rgba, fr.d_depth, fr.d_err, fr.d_n):
                assert bool((t == SENTINEL).all())
            assert bool((fr.d_slots == listed).all()) and not fr.counters().any()

        both = ((lambda **kw: fr.pass_call(n_list, 2, **kw)), (lambda **kw: fr.select_call(0.1, 2, **kw)))
        for call in both:
            untouched(call(params=params_of(sc, spp=SPP // 2)), R.RT_E_ARG)      # not the scene's spp
            untouched(call(params=params_of(sc, width=0)), R.RT_E_ARG)
            for null in ("d_state", "d_aux", "d_tiles", "d_slots"):
                untouched(call(**{null: None}), R.RT_E_ARG)
            for n, T in ((0, 16), (-1, 16), (2, 8), (2, 24), (2, 0), ((1 << 21) + 1, 32)):
                untouched(call(n_tiles=n, T=T), R.RT_E_ARG)
            untouched(call(params=params_of(sc, show_normal=1)), R.RT_E_UNSUPPORTED)
            untouched(call(params=params_of(sc, show_normal=1), d_aux=None), R.RT_E_ARG)   # argument errors first
        untouched(fr.select_call(0.1, 2, d_n_active=None), R.RT_E_ARG)
        untouched(fr.pass_call((1 << 31) + 1, 2), R.RT_E_ARG)
        untouched(fr.pass_call(0, 2), R.RT_OK)                                             # nothing launched
        untouched(fr.pass_call(0, 2, d_slots=None), R.RT_OK)
        untouched(fr.pass_call(n_list, 0), R.RT_OK)
        aux = fr.aux().copy()                                                              # and the scene still renders
        aux[fr.inside] = np.zeros(1, R.PASS_AUX_DTYPE)
        fr.set_aux(aux)
        assert fr.run_pass(n_list, SPP, d_out=None, d_depth=None, d_counters=None) == R.RT_OK   # null outputs
        assert np.all(fr.aux()["count"][fr.inside] == SPP)
        assert bool((fr.d_rgba == SENTINEL).all()) and bool((fr.d_depth == SENTINEL).all())
    finally:
        R.load().rt_dev_scene_free(s)


# DESIGN.md 5.17's table: which -> (VGPRs, static LDS bytes, resident 256-lane blocks per CU)
RESOURCES = {24: (31, 0, 8), 25: (39, 0, 8), 26: (145, 71936, 2), 27: (150, 53248, 3), 28: (21, 32, 8), 30: (20, 32, 8)}


def test_kernel_resources(gpu):
    """The tile-list instances as loaded: no scratch, and the registers, LDS and occupancy of DESIGN.md 5.17's
    table."""
    infos = {which: R.pass_kernel_info(which) for which in RESOURCES}
    for which, info in infos.items():
        print(R.ADAPTIVE_TILE_KERNELS[which], info)
    for which, want in RESOURCES.items():
        info = infos[which]
        assert info["scratch_bytes"] == 0, which
        assert (info["vgprs"], info["lds_bytes"], info["blocks_per_cu"]) == want, which
