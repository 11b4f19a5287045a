"""tests/adaptive_ref.py against tests/pass_ref.py (whose full folds tests/test_pass_ref.py ties to the oracle's
frames): with tol < 0 the loop is the uniform passes; a pixel that stopped at n samples holds pass_ref's
state after n; and the (batch, tol) the GPU tests use are not degenerate on the fixtures."""
import numpy as np
import pytest

import adaptive_ref as A
import pass_ref as PR

NAMES = PR.INW + [PR.IOW]


def same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


@pytest.mark.parametrize("name", NAMES)
def test_negative_tol_is_the_uniform_passes(name):
    spp = PR.spp_of(name)
    batch = A.SETTINGS[name][0]
    rounds = A.loop(name, batch, -1.0)
    assert len(rounds) == -(-spp // batch)
    for i, r in enumerate(rounds):
        k = min((i + 1) * batch, spp)
        want = PR.state(name, k)
        assert np.all(r["aux"]["count"] == k)
        assert same(r["state"], want)
        rgba, depth = PR.image(want, k)
        assert same(r["rgba"], rgba) and same(r["depth"], depth)
        assert r["n_active"] == (A.W * A.H if k < spp else 0)
        assert r["counters"] == PR.counters(name, i * batch, k)
    last = rounds[-1]
    assert np.all(last["list"]["x"] == -1) and np.all(last["list"]["y"] == -1) and len(last["list"]) == A.W * A.H


@pytest.mark.parametrize("name", NAMES)
def test_every_final_count_holds_the_prefix_state(name):
    batch, tol = A.SETTINGS[name]
    last = A.loop(name, batch, tol)[-1]
    count = last["aux"]["count"]
    assert last["n_active"] == 0
    for n in np.unique(count):
        m = count == n
        want = PR.state(name, int(n))
        assert same(last["state"][m], want[m]), n
        rgba, depth = PR.image(want, int(n))
        assert same(last["rgba"][m], rgba[m]) and same(last["depth"][m], depth[m]), n
        # even: the fold over the even samples alone, from scratch
        assert same(last["aux"]["even"][m], A.fold_even(name, PR.samples(name)[m], 0, int(n))), n


@pytest.mark.parametrize("name", NAMES)
def test_settings_are_not_degenerate(name):
    batch, tol = A.SETTINGS[name]
    spp = PR.spp_of(name)
    rounds = A.loop(name, batch, tol)
    count = rounds[-1]["aux"]["count"]
    values, pixels = np.unique(count, return_counts=True)
    print(name, dict(zip(values.tolist(), pixels.tolist())))
    n = count.size
    assert len(values) >= 3
    assert (count < spp).sum() >= 0.1 * n
    assert (count > batch).sum() >= 0.1 * n
    assert len(rounds) >= 3


def test_unit_order_and_tail():
    x, y = A.unit_order(16, 9)
    assert len(x) == 144 and len(set(zip(x.tolist(), y.tolist()))) == 144
    assert (x[0], y[0]) == (0, 0) and (x[7], y[7]) == (7, 0) and (x[8], y[8]) == (0, 1)
    assert (x[64], y[64]) == (8, 0)           # the second 8x8 block
    assert (x[128], y[128]) == (0, 8)         # the second block row holds one pixel row of the 9
    x, y = A.unit_order(37, 23, (5, 3, 20, 11))
    assert len(x) == 220 and x.min() == 5 and x.max() == 24 and y.min() == 3 and y.max() == 13
    x, y = A.unit_order(16, 9, (10, 5, 20, 11))  # a rectangle that leaves the image is clipped
    assert len(x) == 6 * 4


def test_error_and_active_rule():
    st = np.zeros(6, PR.STATE_DTYPE)
    aux = np.zeros(6, A.AUX_DTYPE)
    st["acc"] = [[3, 3, 3], [1, 1, 1], [4, 2, 0], [np.nan, 0, 0], [np.inf, 0, 0], [8, 8, 8]]
    aux["even"] = [[2, 2, 2], [1, 1, 1], [2, 1, 1], [0, 0, 0], [1, 0, 0], [4, 4, 4]]
    aux["count"] = [3, 1, 4, 2, 2, 8]
    act, err = A.active(st, aux, 0.5, 2, 8)
    assert err[0] == 0.0 and np.isinf(err[1]) and err[2] == np.float32(0.5) and np.isnan(err[3]) and np.isinf(err[4])
    assert act.tolist() == [False, True, False, True, True, False]   # NaN and inf keep sampling; n == S stops
    assert A.active(st, aux, -1.0, 0, 8)[0].tolist() == [True] * 5 + [False]  # tol < 0: active until S
    assert A.active(st, aux, 10.0, 4, 8)[0].tolist() == [True, True, False, True, True, False]  # min_samples
