"""The walk-trip fixtures (tests/golden/trace_walk_*.npz) on the CPU: tests/trace_ref.c recomputes
every one bit for bit, and each still holds the cases tests/test_gpu_walk_trip.py needs it for
(tests/walk_trip_cases.py: overflowing lanes beside others, refused lanes, two time bins, hits at
the leaf-box entry, ...), checked with the host-built walk structures and a model of the walk's
stack -- no GPU."""
import numpy as np
import pytest

import trace_ref as T
import walk_trip_cases as W


@pytest.fixture(scope="module")
def ref_lib(tmp_path_factory):
    return T.build(tmp_path_factory.mktemp("trace_ref_walk"))


@pytest.mark.parametrize("name", W.FIXTURES)
def test_fixture_recomputes_bit_for_bit(ref_lib, name):
    fx = T.load_fixture(name)
    n = fx["geom"].shape[0]
    assert fx["geom"].shape == (n, 28) and fx["nodes"].shape == (2 * n - 1, 8) and fx["aabbs"].shape == (n, 6)
    assert 64 < len(fx["rays"]) <= 2048 and fx["layout"] == 1
    for inv in (0, 1):
        hits, ctr = T.run(ref_lib, fx["geom"], fx["nodes"], fx["layout"], fx["rays"], inv)
        assert T.same_hits(hits, fx[f"hits{inv}"]), (name, inv)
        assert np.array_equal(ctr, fx[f"ctr{inv}"]), (name, inv)
        assert int(ctr[2]) == 0  # the reference's own stack drops nothing: the wide walk is allowed


@pytest.mark.parametrize("name", W.FIXTURES)
def test_fixture_holds_its_cases(name):
    print(name, W.check(name, T.load_fixture(name)))


def test_walk_model_counts_a_known_stack():
    """The stack model on a hand-made node: three hit leaves and a culled slot."""
    wn = np.zeros((1, 40), np.float32)
    for c, x in enumerate((1.0, 3.0, 5.0, 1e30)):
        lo, hi = (x, -1.0, -1.0), (x + 1.0, 1.0, 1.0)
        for a in range(3):
            wn[0, 4 * a + c] = wn[0, 24 + 4 * a + c] = lo[a] if x < 1e29 else 1e30
            wn[0, 4 * (a + 3) + c] = hi[a] if x < 1e29 else 1e30
    links = np.array([[-2, 0, -1, 10 ** 9]], np.int32)
    o, d = np.array([0.0, 0.1, 0.1], np.float32), np.array([1.0, 1e-3, 1e-3], np.float32)
    over, high, steps = W.walk_model(wn, links, 1, o, d, 32000.0)
    assert (over, high, steps) == (False, 2, 1)
    assert W.walk_model(wn, links, 1, o, d, 32000.0, cap=1)[0]
    assert W.walk_model(wn, links, 1, o, -d, 32000.0) == (False, 0, 1)  # everything behind the ray
