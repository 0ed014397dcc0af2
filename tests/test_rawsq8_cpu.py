"""CPU: the scalar-quantised raw store's host code and model key.  gamma_hip_raw_sq8_params and gamma_hip_raw_sq8_check (pure
host code: no handle, no device) against the numpy restatement of the contract (tests/sq8_ref.py), the restatement's own two
properties, and the value "sq8" of the HIP-only model key "raw_dtype"."""
import ctypes as C

import numpy as np
import pytest

from gamma_amd import _lib, plugin
from tests import sq8_ref as S

BASE = '"ncentroids": 16, "nsubvector": 8'
OK, EINVAL = 0, -1   # include/gamma_hip.h
F = np.float32


def _p(a):
    return a.ctypes.data_as(_lib.f32p)


def _params(vmin, vmax):
    vmin, vmax = np.ascontiguousarray(vmin, F), np.ascontiguousarray(vmax, F)
    step, inv = np.full(len(vmin), 7.0, F), np.full(len(vmin), 7.0, F)
    rc = _lib.load().gamma_hip_raw_sq8_params(len(vmin), _p(vmin), _p(vmax), _p(step), _p(inv))
    return rc, step, inv


def _check(x):
    x = np.ascontiguousarray(x, dtype=F)
    bad = C.c_int64(-7)
    return _lib.load().gamma_hip_raw_sq8_check(_p(x), x.size, C.byref(bad)), bad.value


# ---- params -----------------------------------------------------------------------------------------------------------
def _ranges(seed, d=64):
    """ranges of magnitudes 1e-3 .. 1e3, a third of them negative throughout, some straddling zero"""
    rng = np.random.default_rng(seed)
    mag = 10.0 ** rng.uniform(-3, 3, d)
    lo = (rng.uniform(-1, 1, d) * mag).astype(F)
    hi = (lo + (rng.uniform(0.01, 2, d) * mag).astype(F)).astype(F)
    neg = np.arange(d) % 3 == 0
    lo[neg], hi[neg] = -np.abs(hi[neg]) - np.abs(lo[neg]) - F(1e-3), -np.abs(lo[neg]) - F(1e-3)
    assert (lo <= hi).all()
    return lo, hi


@pytest.mark.parametrize("seed", range(6))
def test_params_equal_the_restatement_bit_for_bit(seed):
    vmin, vmax = _ranges(seed)
    assert (vmax[::3] < 0).all()
    step, inv = S.params(vmin, vmax)
    rc, s, i = _params(vmin, vmax)
    assert rc == OK and s.tobytes() == step.tobytes() and i.tobytes() == inv.tobytes()
    assert (step > 0).all() and (inv > 0).all()


def test_params_of_constant_and_nearly_constant_dimensions():
    tiny = np.nextafter(F(0), F(1))                                       # the smallest subnormal: 255 / span overflows
    vmin = np.array([0.75, -2.5, 0.0, 0.0, 1.0, -3e38, -1e-3], F)
    vmax = np.array([0.75, -2.5, tiny, 1e-35, np.nextafter(F(1), F(2)), 3e37, 1e3], F)
    step, inv = S.params(vmin, vmax)
    assert step[0] == 0 and inv[0] == 0 and step[1] == 0 and inv[1] == 0   # span 0
    assert step[2] == 0 and inv[2] == 0                                    # inv would be infinite
    assert inv[3] > 0 and np.isfinite(inv[3]) and inv[4] > 0 and inv[5] > 0
    rc, s, i = _params(vmin, vmax)
    assert rc == OK and s.tobytes() == step.tobytes() and i.tobytes() == inv.tobytes()
    # either output may be null
    L = _lib.load()
    assert L.gamma_hip_raw_sq8_params(len(vmin), _p(vmin), _p(vmax), None, None) == OK


@pytest.mark.parametrize("vmin,vmax", [([0.0, np.nan], [1.0, 1.0]), ([0.0, 0.0], [1.0, np.nan]), ([0.0, -np.inf], [1.0, 1.0]),
                                       ([0.0, 0.0], [1.0, np.inf]), ([0.0, 2.0], [1.0, 1.0]), ([0.0, -3e38], [1.0, 3e38])],
                         ids=["nan_min", "nan_max", "inf_min", "inf_max", "min_above_max", "span_overflows"])
def test_refused_ranges(vmin, vmax):
    with pytest.raises(ValueError):
        S.params(vmin, vmax)
    rc, s, i = _params(vmin, vmax)
    assert rc == EINVAL and (s == 7.0).all() and (i == 7.0).all()         # nothing is written
    assert _lib.load().gamma_hip_raw_sq8_params(0, None, None, None, None) == EINVAL


# ---- the acceptance predicate -------------------------------------------------------------------------------------------
def test_check_accepts_every_finite_value():
    x = np.array([-0.0, 0.0, 1e-45, -1e-45, 3.4e38, -3.4e38, 1e30, -1e30, 0.5, 255.0, 256.0], F)
    assert np.isfinite(x).all() and _check(x) == (OK, -7)
    assert _check(x[:0]) == (OK, -7)


def test_check_reports_the_first_non_finite_position():
    good = np.random.default_rng(3).standard_normal(1000).astype(F) * F(1e20)
    for v in (np.nan, np.inf, -np.inf):
        for pos in (0, 1, 499, 999):
            x = good.copy()
            x[pos] = v
            x[min(pos + 3, 999)] = np.nan                      # a later one does not matter
            assert _check(x) == (EINVAL, pos)
    x = good.copy()
    x[17] = np.inf
    assert _lib.load().gamma_hip_raw_sq8_check(_p(x), x.size, None) == EINVAL   # a null first_bad is allowed


# ---- the restatement's own properties -----------------------------------------------------------------------------------
def test_error_bound_and_code_round_trip():
    """200 random scale / offset settings, ranges from half of the rows, the other half drawn wider so that values clip:
    |w - clip(x, vmin, vmax)| <= step / 2 + 4 * 2^-23 * max(|vmin|, |vmax|) (half a step of the grid plus the roundings of the
    four fp32 operations at the range's magnitude), and encode(decode(c)) == c for every code of every dimension."""
    rng = np.random.default_rng(42)
    worst = 0.0
    codes = np.arange(256, dtype=np.uint8)[:, None]
    for _ in range(200):
        d = 16
        scale = 10.0 ** rng.uniform(-3, 3, d)
        offset = rng.uniform(-10, 10, d) * scale
        a = (offset + scale * rng.standard_normal((400, d))).astype(F)
        b = (offset + 2.0 * scale * rng.standard_normal((400, d))).astype(F)
        a[:, 3] = a[0, 3]                                                   # a constant dimension
        vmin, vmax = a.min(axis=0), a.max(axis=0)
        step, inv = S.params(vmin, vmax)
        x = np.concatenate([a, b])
        c = S.encode(x, vmin, inv)
        w = S.decode(c, vmin, step)
        assert (c[:, 3] == 0).all() and (w[:, 3] == vmin[3]).all()
        assert c.min() == 0 and c.max() == 255
        clip = np.clip(x.astype(np.float64), vmin.astype(np.float64), vmax.astype(np.float64))
        bound = 0.5 * step.astype(np.float64) + 4 * 2.0 ** -23 * np.maximum(np.abs(vmin), np.abs(vmax)).astype(np.float64)
        live = inv != 0
        err = np.abs(w.astype(np.float64) - clip)
        assert (err[:, live] <= bound[live]).all()
        worst = max(worst, float((err[:, live] / bound[live]).max()))
        back = S.encode(S.decode(np.broadcast_to(codes, (256, d)), vmin, step), vmin, inv)
        assert (back[:, live] == codes).all() and (back[:, ~live] == 0).all()
    assert worst <= 1.0


def test_encode_rounds_half_to_even_and_clips():
    vmin, vmax = np.array([0.0], F), np.array([255.0], F)               # step = inv = 1
    step, inv = S.params(vmin, vmax)
    assert step[0] == 1 and inv[0] == 1
    x = np.array([[0.5], [1.5], [2.5], [254.5], [-0.0], [-7.0], [300.0], [3e38], [-3e38]], F)
    assert S.encode(x, vmin, inv).reshape(-1).tolist() == [0, 2, 2, 254, 0, 0, 255, 255, 0]


# ---- the model key --------------------------------------------------------------------------------------------------------
def _parse(extra=""):
    return plugin.parse_raw_dtype("{%s%s}" % (BASE, extra))   # (loads the host library: a missing one is a failure)


def test_sq8_is_accepted_in_any_case_and_answers_4():
    assert _parse(', "raw_dtype": "sq8"') == (0, "sq8")
    assert _parse(', "raw_dtype": "SQ8"') == (0, "sq8")
    assert _parse(', "raw_dtype": "Sq8"') == (0, "sq8")
    out = (C.c_int * 2)()
    plugin.load_host().gh_parse_ivfpq_raw_dtype(('{%s, "raw_dtype": "SQ8"}' % BASE).encode(), out)
    assert (out[0], out[1]) == (0, 4)
    s = '{%s, "raw_dtype": "sq8", "nprobe": 4, "metric_type": "L2"}' % BASE
    p = plugin.parse_model_params(s)
    assert p["rc"] == 0 and p["ncentroids"] == 16 and p["nsubvector"] == 8 and p["nprobe"] == 4


def test_near_misses_are_rejected_and_the_other_answers_unchanged():
    for value in ('"sq4"', '"sq"', '"scalar8"', '"sq8 "', '"sq16"'):
        assert _parse(', "raw_dtype": %s' % value)[0] == -1
        assert plugin.parse_model_params('{%s, "raw_dtype": %s}' % (BASE, value))["rc"] == -1
    assert _parse() == (0, "float32")
    assert _parse(', "raw_dtype": "float16"') == (0, "float16")
    assert _parse(', "raw_dtype": "uint8"') == (0, "uint8")
    assert _parse(', "raw_dtype": "int8"') == (0, "int8")
    # HIPFLAT and HIPIVFFLAT keep rejecting the value
    assert plugin.parse_flat_raw_dtype('{"raw_dtype": "sq8"}')[0] == -1
    assert plugin.parse_ivfflat_raw_dtype('{"ncentroids": 16, "raw_dtype": "sq8"}')[0] == -1
