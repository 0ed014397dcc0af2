"""The margin of the coarse quantizer's bf16 filter (csrc/coarse.hip, "bf16 filter"), checked on the CPU: a numpy
emulation of the split (hi = bf16(x) to nearest even, lo = bf16(x - hi)) and of the three products with fp32
accumulation, against the oracle's GEMM-form knn_L2sqr distances.  The constant is parsed from csrc/kernels.h, the
place the kernels take it from."""
import os
import re

import numpy as np
import pytest

from gamma_amd import synth
from oracle import binding as B

_KH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gamma_amd", "csrc", "kernels.h")


def _constant(name):
    m = re.search(r"constexpr float %s = ([0-9.eE+-]+)f;" % name, open(_KH).read())
    assert m, name
    return np.float32(float(m.group(1)))


C = _constant("kCoarseBfMargin")
NQ, NY, D, P = 256, 1024, 128, 32


def _bf16(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u >> 16) & 1) + 0x7FFF
    return ((u + r) & 0xFFFF0000).astype(np.uint32).view(np.float32)


def _split(x):
    hi = _bf16(x)
    return hi, _bf16(x - hi)


def _approx(x, y):
    """d~ = fma(-2, ip~, xn~ + yn) with ip~ = xh.yh + xh.yl + xl.yh accumulated in fp32 (here: fp32 matrix products,
    the -2 ip~ product is exact)"""
    xh, xl = _split(x)
    yh, yl = _split(y)
    ip = (xl @ yh.T + xh @ yl.T + xh @ yh.T).astype(np.float32)
    xn = np.einsum("ij,ij->i", x, x, dtype=np.float32)
    yn = np.einsum("ij,ij->i", y, y, dtype=np.float32)
    s = (xn[:, None] + yn[None, :]).astype(np.float32)
    dt = (s.astype(np.float64) - 2.0 * ip.astype(np.float64)).astype(np.float32)
    return dt, s


def _exact(x, y):
    Ds, Is = B.knn_L2sqr(x, y, y.shape[0], mode=1)
    out = np.empty_like(Ds)
    np.put_along_axis(out, Is, Ds, axis=1)
    return out


def _cases():
    rng = np.random.default_rng(5)
    g_y = (rng.standard_normal((NY, D)) * 20).astype(np.float32)
    g_x = (g_y[rng.integers(0, NY, NQ)] + rng.standard_normal((NQ, D)) * 12).astype(np.float32)
    base = synth.sift_like(NY + NQ, d=D, seed=31)
    off_y, off_x = g_y + np.float32(1000), g_x + np.float32(1000)
    c_y = (rng.standard_normal((NY, D)) * 300).astype(np.float32)
    c_y[NY // 2:] = c_y[:NY // 2] + (rng.standard_normal((NY // 2, D)) * 1e-3).astype(np.float32)
    c_x = (c_y[rng.integers(0, NY, NQ)] + rng.standard_normal((NQ, D)) * 1e-2).astype(np.float32)
    return {"gaussian": (g_x, g_y), "sift_like": (base[NY:], base[:NY]), "offset": (off_x, off_y),
            "cancellation": (c_x, c_y)}


@pytest.fixture(scope="module")
def computed():
    out = {}
    for name, (x, y) in _cases().items():
        dt, s = _approx(x, y)
        out[name] = (dt, s, _exact(x, y))
    return out


@pytest.mark.parametrize("name", ["gaussian", "sift_like", "offset", "cancellation"])
def test_error_within_the_kernels_constant(computed, name):
    dt, s, ex = computed[name]
    # the exact path clamps at 0; the approximation is compared before the clamp, which only moves exact towards it
    err = np.abs(dt.astype(np.float64) - ex.astype(np.float64))
    neg = (ex == 0) & (dt < 0)
    err[neg] = 0
    rel = (err / np.maximum(s.astype(np.float64), 1e-300)).max()
    print(name, "max |d~ - exact| / (xn + yn) =", rel, "constant", float(C))
    assert rel <= float(C)
    if name == "sift_like":
        assert rel == 0.0       # 16 bits of hi + lo hold the integers, all sums stay below 2^24


@pytest.mark.parametrize("name", ["gaussian", "sift_like", "offset", "cancellation"])
def test_selection_invariant(computed, name):
    """kb = a bound with P approximations <= kb (here the tightest: the P-th smallest).  Then every entry whose exact
    value is <= the P-th smallest exact value T -- ties at T included -- has approximation <= kb + 2 eps_qc."""
    dt, s, ex = computed[name]
    eps = (float(C) * s.astype(np.float64))
    kb = np.sort(dt, axis=1)[:, P - 1].astype(np.float64)
    T = np.sort(ex, axis=1)[:, P - 1]
    needed = ex <= T[:, None]
    kept = dt.astype(np.float64) <= kb[:, None] + 2 * eps
    assert not (needed & ~kept).any()
    # and the form the kernels use: L = d~ - eps is a lower bound of the exact value, L + 2 eps an upper bound
    L = dt.astype(np.float64) - eps
    assert (L <= ex).all() and (ex <= L + 2 * eps).all()
