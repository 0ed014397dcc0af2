"""CPU: the values "uint8" / "int8" of the HIP-only model key "raw_dtype" (HIPIVFPQModelParams::Parse), and the byte store's
acceptance predicate gamma_hip_raw_i8_check (pure host code: no handle, no device) against its numpy restatement."""
import ctypes as C

import numpy as np
import pytest

from gamma_amd import _lib, plugin

BASE = '"ncentroids": 16, "nsubvector": 8'
OK, EINVAL = 0, -1   # include/gamma_hip.h
RANGE = {0: (0.0, 255.0), 1: (-128.0, 127.0)}


def _parse(extra=""):
    return plugin.parse_raw_dtype("{%s%s}" % (BASE, extra))   # (loads the host library: a missing one is a failure)


def test_byte_types_are_accepted_in_any_case():
    assert _parse(', "raw_dtype": "uint8"') == (0, "uint8")
    assert _parse(', "raw_dtype": "int8"') == (0, "int8")
    assert _parse(', "raw_dtype": "UInt8"') == (0, "uint8")
    assert _parse(', "raw_dtype": "INT8"') == (0, "int8")


def test_the_other_answers_are_unchanged():
    assert _parse() == (0, "float32")
    assert _parse(', "raw_dtype": "float32"') == (0, "float32")
    assert _parse(', "raw_dtype": "float16"') == (0, "float16")
    assert _parse(', "raw_dtype": "Float16"') == (0, "float16")
    for value in ('"bfloat16"', '"uint4"', '"int16"', '"u8"', '""'):
        assert _parse(', "raw_dtype": %s' % value)[0] == -1


def test_the_other_keys_parse_beside_it():
    s = '{%s, "raw_dtype": "int8", "nprobe": 4, "metric_type": "L2"}' % BASE
    assert plugin.parse_raw_dtype(s) == (0, "int8")
    p = plugin.parse_model_params(s)
    assert p["rc"] == 0 and p["ncentroids"] == 16 and p["nsubvector"] == 8 and p["nprobe"] == 4


def _check(x, is_signed):
    x = np.ascontiguousarray(x, dtype=np.float32)
    bad = C.c_int64(-7)
    rc = _lib.load().gamma_hip_raw_i8_check(x.ctypes.data_as(_lib.f32p), x.size, is_signed, C.byref(bad))
    return rc, bad.value


def _storable(x, is_signed):
    lo, hi = RANGE[is_signed]
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return np.isfinite(x) & (x == np.trunc(x)) & (x >= lo) & (x <= hi)


CASES = np.array([-0.0, 255.5, 256.0, -1.0, -129.0, 128.0, 1e-3, np.nan, np.inf, -np.inf, 3e38, -3e38, 0.0, 255.0, -128.0, 127.0,
                  0.5, -0.5, 254.99998, -128.00002, 1e-45, 2.0 ** 31, -2.0 ** 31, 2.0 ** 32 + 256], dtype=np.float32)


@pytest.mark.parametrize("is_signed", [0, 1], ids=["uint8", "int8"])
def test_every_value_of_the_type_is_accepted(is_signed):
    lo, hi = RANGE[is_signed]
    allv = np.arange(lo, hi + 1, dtype=np.float32)
    assert len(allv) == 256 and _storable(allv, is_signed).all()
    assert _check(allv, is_signed) == (OK, -7)                 # first_bad is left alone
    assert _check(allv[:0], is_signed) == (OK, -7)
    # and as the bytes they become, the widening gives them back
    t = np.int8 if is_signed else np.uint8
    assert np.array_equal(allv.astype(t).astype(np.float32), allv)


@pytest.mark.parametrize("is_signed", [0, 1], ids=["uint8", "int8"])
def test_single_values_against_numpy(is_signed):
    want = _storable(CASES, is_signed)
    # what the contract says about its own examples
    assert want[0]                                             # -0.0 is accepted
    assert not want[1] and not want[2] and not want[6:11].any()  # 255.5, 256, 1e-3, NaN, +-inf, 3e38
    assert want[3] == bool(is_signed) and not want[4] and want[5] == (not is_signed)   # -1, -129, 128
    for v, ok in zip(CASES, want):
        rc, bad = _check([v], is_signed)
        assert (rc, bad) == ((OK, -7) if ok else (EINVAL, 0)), (float(v), rc, bad)


@pytest.mark.parametrize("is_signed", [0, 1], ids=["uint8", "int8"])
def test_first_bad_is_the_first_refused_value(is_signed):
    lo, hi = RANGE[is_signed]
    rng = np.random.default_rng(5 + is_signed)
    good = rng.integers(int(lo), int(hi) + 1, size=1000).astype(np.float32)
    for v in CASES[~_storable(CASES, is_signed)]:
        for pos in (0, 1, 499, 999):
            x = good.copy()
            x[pos] = v
            x[min(pos + 3, 999)] = v                           # a later one does not matter
            assert _check(x, is_signed) == (EINVAL, pos)
    x = np.concatenate([good, CASES, good])
    want = _storable(x, is_signed)
    assert _check(x, is_signed) == (EINVAL, int(np.argmin(want)))
    # a null first_bad is allowed
    assert _lib.load().gamma_hip_raw_i8_check(x.ctypes.data_as(_lib.f32p), x.size, is_signed, None) == EINVAL
