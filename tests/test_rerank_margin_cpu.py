"""The bound of the re-rank filter (csrc/rerank_filter.hip), checked on the CPU: a numpy fp32 emulation of the image (lo, Delta,
the byte rows, err, nrm), of the kernel's estimate and of its lb / ub, against the reference's 8-lane fma chain (fvec_L2sqr /
fvec_inner_product as csrc/rerank_dev.h runs it; tests/rerank_ref.py exact_chain) and against the value in float64.
lb <= exact <= ub for every (query, row) pair, at the row lengths the kernel admits: 16 (one piece, seven idle lanes), 128 (the
register form), 272 (lanes with one piece more than others), 768 and 1536 (kRerankFilterMaxD: n of the error analysis at its
largest).  The margin is parsed from csrc/kernels.h, the place the kernel takes it from."""
import os
import re

import numpy as np
import pytest

from gamma_amd import synth
from tests.rerank_ref import exact_chain as _exact, fma32 as _fma

_KH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gamma_amd", "csrc", "kernels.h")
F = np.float32


def _constant(name):
    m = re.search(r"constexpr float %s = ([0-9.eE+-]+)f;" % name, open(_KH).read())
    assert m, name
    return np.float32(float(m.group(1)))


M = _constant("kRerankFilterMargin")


def _sizes(d):
    """(queries, rows): the emulation holds nq x ny x d arrays"""
    return (48, 768) if d < 768 else (8, 256)


def _group8(a):
    """a[..., 8] -> the kernel's a += down 4, += down 2, + down 1 on lane 0"""
    s = a[..., :4] + a[..., 4:]
    s = s[..., :2] + s[..., 2:]
    return s[..., 0] + s[..., 1]


def _chain16(term, acc_of):
    """term[..., d] laid out as the filter reads it: lane l owns the 16-element pieces l, l + 8, ..; acc_of(acc, piece element)"""
    d = term.shape[-1]
    nc = d // 16
    acc = np.zeros(term.shape[:-1] + (8,), F)
    for c0 in range(0, nc, 8):
        for e in range(16):
            for l in range(min(8, nc - c0)):
                acc[..., l] = acc_of(acc[..., l], term[..., 16 * (c0 + l) + e])
    return _group8(acc)


def _image(y):
    lo = y.min(axis=0).astype(F)
    span = (y.max(axis=0).astype(F) - lo).astype(F)
    whole = bool(np.all(lo == np.rint(lo)) and np.all(span == np.rint(span)))
    delta = F(span.max() / F(255.0))
    if not (delta > 0 and np.isfinite(delta)) or (whole and span.max() <= 255):
        delta = F(1.0)
    return _image_with(y, lo, delta)


def _bounds(x, im, l2):
    lo, delta, u = im["lo"], im["delta"], im["u"]
    if l2:
        xp = (x - lo).astype(F)
        xn = (np.sqrt(np.sum(xp * xp, axis=1, dtype=F)) * (F(1) + M)).astype(F)
        t = _fma(np.full((x.shape[0],) + u.shape, -delta, F), np.broadcast_to(u[None], (x.shape[0],) + u.shape),
                 np.broadcast_to(xp[:, None, :], (x.shape[0],) + u.shape))
        est = _chain16(t, lambda acc, v: _fma(v, v, acc))
        rt = np.sqrt(est).astype(F)
        slack = _fma(np.full_like(rt, M), (rt + xn[:, None]).astype(F), np.broadcast_to(im["err"][None], rt.shape))
        ur, lr = (rt + slack).astype(F), np.maximum((rt - slack).astype(F), F(0))
        return ((lr * lr).astype(F) * (F(1) - M)).astype(F), ((ur * ur).astype(F) * (F(1) + M)).astype(F)
    xn = (np.sqrt(np.sum(x * x, axis=1, dtype=F)) * (F(1) + M)).astype(F)
    c0 = np.sum(x * lo, axis=1, dtype=F)
    shape = (x.shape[0],) + u.shape
    prod = np.stack([np.broadcast_to(x[:, None, :], shape), np.broadcast_to(u[None], shape)])
    acc = np.zeros(shape[:-1] + (8,), F)
    nc = u.shape[-1] // 16
    for cc in range(0, nc, 8):
        for e in range(16):
            for l in range(min(8, nc - cc)):
                j = 16 * (cc + l) + e
                acc[..., l] = _fma(prod[0][..., j], prod[1][..., j], acc[..., l])
    est = _fma(np.full(shape[:-1], delta, F), _group8(acc), np.broadcast_to(c0[:, None], shape[:-1]))
    inner = _fma(np.full_like(im["nrm"], M), (im["nrm"] + im["lon"]).astype(F), im["err"])
    slack = (xn[:, None] * inner[None, :]).astype(F)
    return (est - slack).astype(F), (est + slack).astype(F)


def _cases(d):
    NQ, NY = _sizes(d)
    rng = np.random.default_rng(5 + d)
    g_y = (rng.standard_normal((NY, d)) * 20).astype(F)
    g_x = (g_y[rng.integers(0, NY, NQ)] + rng.standard_normal((NQ, d)) * 12).astype(F)
    base = synth.sift_like(NY + NQ, d=d, seed=31)
    c_y = (rng.standard_normal((NY, d)) * 300).astype(F)
    c_y[NY // 2:] = c_y[:NY // 2] + (rng.standard_normal((NY // 2, d)) * 1e-3).astype(F)
    c_x = (c_y[rng.integers(0, NY, NQ)] + rng.standard_normal((NQ, d)) * 1e-2).astype(F)
    # the rows of the GPU legs (tests/test_gpu_rerank_filter_shapes.py): standard normal * 20 + 1000 in fp32, lo != 0 and
    # x - lo cancels; queries of the same kind, unrelated to the rows
    s_y = (rng.standard_normal((NY, d)).astype(F) * F(20) + F(1000)).astype(F)
    s_x = (rng.standard_normal((NQ, d)).astype(F) * F(20) + F(1000)).astype(F)
    # magnitudes around 1e15 (squares and their sums over 1536 elements stay finite): u |x - lo| against a large lo
    h_y = (F(1e15) + rng.standard_normal((NY, d)).astype(F) * F(3e13)).astype(F)
    h_x = (h_y[rng.integers(0, NY, NQ)] + rng.standard_normal((NQ, d)).astype(F) * F(1e13)).astype(F)
    return {"gaussian": (g_x, g_y, g_y), "sift_like": (base[NY:], base[:NY], base[:NY]),
            "offset": (g_x + F(1000), g_y + F(1000), g_y + F(1000)), "cancellation": (c_x, c_y, c_y),
            # the image's range comes from the first rows only: the others clamp
            "clamped": (g_x, g_y, (g_y[:64] * F(0.05)).astype(F)),
            "scaled_shifted": (s_x, s_y, s_y), "huge": (h_x, h_y, h_y)}


@pytest.mark.parametrize("l2", [True, False])
@pytest.mark.parametrize("name", ["gaussian", "sift_like", "offset", "cancellation", "clamped", "scaled_shifted", "huge"])
@pytest.mark.parametrize("d", [16, 128, 272, 768, 1536])
def test_bounds_hold_for_every_pair(d, name, l2):
    x, y, ranged_on = _cases(d)[name]
    im = _image(y)
    if name == "clamped":
        lim = _image(ranged_on)
        im = _image_with(y, lim["lo"], lim["delta"])
        assert (im["u"] == 0).any() and (im["u"] == 255).any()
    lb, ub = _bounds(x, im, l2)
    ex = _exact(x, y, l2)
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    true = ((x64[:, None, :] - y64[None]) ** 2).sum(-1) if l2 else x64 @ y64.T
    assert (lb <= ex).all() and (ex <= ub).all()
    assert (lb.astype(np.float64) <= true).all() and (true <= ub.astype(np.float64)).all()
    width = float(np.median((ub.astype(np.float64) - lb) / np.maximum(np.abs(true), 1e-30)))
    print(d, name, "L2" if l2 else "IP", "delta", float(im["delta"]), "median (ub - lb) / |exact| =", width)
    if name == "sift_like":
        assert im["delta"] == 1.0 and (np.abs(y - (im["lo"] + im["u"])) == 0).all()   # the image of integer rows is exact


def _image_with(y, lo, delta):
    """the image rows of y under parameters fixed earlier (rows appended after the image was created)"""
    inv = F(F(1.0) / delta)
    yl = (y - lo).astype(F)
    u = np.clip(np.rint((yl * inv).astype(F)), 0, 255).astype(F)
    r = _fma(np.full_like(u, -delta), u, yl)
    sq = lambda acc, v: _fma(v, v, acc)
    sr, syl, sy, su = _chain16(r, sq), _chain16(yl, sq), _chain16(y, sq), _chain16(u, sq)
    err = (_fma(np.full_like(sr, M), np.sqrt(syl), np.sqrt(sr)) * (F(1) + M)).astype(F)
    nrm = (_fma(np.full_like(su, delta), np.sqrt(su), np.sqrt(sy)) * (F(1) + M)).astype(F)
    lon = F(np.sqrt(np.sum(lo * lo, dtype=F)) * (F(1) + M))
    return dict(lo=lo, delta=delta, u=u, err=err, nrm=nrm, lon=lon)
