"""The IOW-03 record packer and RI priors on the host: rt_debug_iow_prepare_host (iow_records and
iow_priors, what rt_dev_scene_iow03 runs) against the numpy restatement of tests/iow_prepare_ref.py, byte
for byte, on every input class the device kernels are later tied to."""
import numpy as np
import pytest

import rt_amd as R
import iow_prepare_ref as P

_cache = {}


def base():
    if "base" not in _cache:
        sc = R.make_scene(R.PRESET_IOW03_FINAL, 20250131, 0, width=48, height=32, spp=6, max_bounces=8)
        assert sc.n == 486
        _cache["base"] = (np.ascontiguousarray(sc.types, np.float32), np.ascontiguousarray(sc.records, np.float32))
    return _cache["base"]


def all_cases():
    if "cases" not in _cache:
        _cache["cases"] = {name: (t, r) for name, t, r in P.cases(*base())}
    return _cache["cases"]


NAMES = ["c2", "first1", "first2", "first3", "ri_equal_7", "ri_tie_7", "ri_eight_7", "ri_nine_7", "ri_equal_1455",
         "ri_tie_1455", "ri_eight_1455", "ri_nine_1455", "edges"]


def test_case_list_is_complete():
    assert sorted(all_cases()) == sorted(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_host_packer_and_priors_match_the_restatement(name):
    types, rec = all_cases()[name]
    got = R.iow_prepare_host(types, rec)
    hot, cold = P.records_ref(types, rec)
    assert got["hot"].tobytes() == hot.tobytes()
    assert got["cold"].tobytes() == cold.tobytes()
    assert got["priors"].tobytes() == P.priors_ref(rec).tobytes(), (got["priors"], P.priors_ref(rec))


def test_priors_of_the_classes():
    """The classes are what they claim: the mode, the tie, the 8 and the 9 patterns."""
    pri = {k: R.iow_prepare_host(*v)["priors"] for k, v in all_cases().items()}
    for n in (7, 1455):
        assert pri[f"ri_equal_{n}"][0] == np.float32(1.5) and pri[f"ri_equal_{n}"][9] == 3.0
        assert list(pri[f"ri_equal_{n}"][1:4]) == [0.0, 1.0, 1.5]
        assert pri[f"ri_tie_{n}"][0] == np.float32(1.3)  # 1.3 and 1.5 equally common
        assert pri[f"ri_eight_{n}"][9] == 8.0 and list(pri[f"ri_eight_{n}"][1:9]) == list(np.array(P.EIGHT, np.float32))
        assert pri[f"ri_nine_{n}"][9] == 0.0 and not pri[f"ri_nine_{n}"][1:9].any()


def test_identity_flag_and_reciprocals_of_the_edge_rows():
    types, rec = all_cases()["edges"]
    hot = R.iow_prepare_host(types, rec)["hot"]
    assert list(hot[:4, 19]) == [1.0, 0.0, 0.0, 0.0]  # exact identity; -0.0 off the diagonal; an ulp off, twice
    assert np.isposinf(hot[4, 16]) and np.isposinf(hot[5, 17])  # 1 / 0 and 1 / subnormal
    assert 0.0 < hot[6, 18] < np.finfo(np.float32).tiny  # 1 / 1e38 is subnormal, not flushed
    assert hot[7, 16] == np.float32(-0.5)


def test_outputs_may_be_null_and_inputs_may_not():
    lib = R.load()
    types, rec = all_cases()["first3"]
    pri = np.zeros(10, np.float32)
    assert lib.rt_debug_iow_prepare_host(R.fptr(types), R.fptr(rec), 3, None, None, R.fptr(pri)) == R.RT_OK
    assert pri.tobytes() == P.priors_ref(rec).tobytes()
    assert lib.rt_debug_iow_prepare_host(R.fptr(types), R.fptr(rec), 3, None, None, None) == R.RT_OK
    assert lib.rt_debug_iow_prepare_host(None, R.fptr(rec), 3, None, None, None) == R.RT_E_ARG
    assert lib.rt_debug_iow_prepare_host(R.fptr(types), None, 3, None, None, None) == R.RT_E_ARG
    assert lib.rt_debug_iow_prepare_host(R.fptr(types), R.fptr(rec), 0, None, None, None) == R.RT_E_ARG
