"""The bound of the re-rank filter (csrc/rerank_filter.hip), checked on the CPU: a numpy fp32 emulation of the image (lo, Delta,
the byte rows, err, nrm), of the kernel's estimate and of its lb / ub, against the reference's 8-lane fma chain (fvec_L2sqr /
fvec_inner_product as csrc/rerank_dev.h runs it) and against the value in float64.  lb <= exact <= ub for every (query, row)
pair.  The margin is parsed from csrc/kernels.h, the place the kernel takes it from."""
import os
import re

import numpy as np
import pytest

from gamma_amd import synth

_KH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gamma_amd", "csrc", "kernels.h")
F = np.float32


def _constant(name):
    m = re.search(r"constexpr float %s = ([0-9.eE+-]+)f;" % name, open(_KH).read())
    assert m, name
    return np.float32(float(m.group(1)))


M = _constant("kRerankFilterMargin")
NQ, NY = 48, 768


def _fma(a, b, c):
    """fp32 fma: the product of two floats is exact in float64"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


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


def _exact(x, y, l2):
    """the reference's chain: lane l runs elements l, l + 8, ..; s[l] = acc[l + 4] + acc[l]; (s0 + s1) + (s2 + s3)"""
    d = x.shape[-1]
    acc = np.zeros((x.shape[0], y.shape[0], 8), F)
    for i in range(0, d, 8):
        xs, ys = x[:, None, i:i + 8], y[None, :, i:i + 8]
        if l2:
            t = (xs - ys).astype(F)
            acc = _fma(t, t, acc)
        else:
            acc = _fma(np.broadcast_to(xs, acc.shape), np.broadcast_to(ys, acc.shape), acc)
    s = acc[..., 4:] + acc[..., :4]
    return (s[..., 0] + s[..., 1]) + (s[..., 2] + s[..., 3])


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
    rng = np.random.default_rng(5 + d)
    g_y = (rng.standard_normal((NY, d)) * 20).astype(F)
    g_x = (g_y[rng.integers(0, NY, NQ)] + rng.standard_normal((NQ, d)) * 12).astype(F)
    base = synth.sift_like(NY + NQ, d=d, seed=31)
    c_y = (rng.standard_normal((NY, d)) * 300).astype(F)
    c_y[NY // 2:] = c_y[:NY // 2] + (rng.standard_normal((NY // 2, d)) * 1e-3).astype(F)
    c_x = (c_y[rng.integers(0, NY, NQ)] + rng.standard_normal((NQ, d)) * 1e-2).astype(F)
    return {"gaussian": (g_x, g_y, g_y), "sift_like": (base[NY:], base[:NY], base[:NY]),
            "offset": (g_x + F(1000), g_y + F(1000), g_y + F(1000)), "cancellation": (c_x, c_y, c_y),
            # the image's range comes from the first rows only: the others clamp
            "clamped": (g_x, g_y, (g_y[:64] * F(0.05)).astype(F))}


@pytest.mark.parametrize("l2", [True, False])
@pytest.mark.parametrize("name", ["gaussian", "sift_like", "offset", "cancellation", "clamped"])
@pytest.mark.parametrize("d", [128, 272])
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
