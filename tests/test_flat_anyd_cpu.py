"""CPU: the shapes and margins of the flat search's matrix-pipe filter for any row length (csrc/flat_mfma.hip, DESIGN section
19), read from gamma_hip_flat_filter_shape -- no device call -- and the split claim the margin rests on, under padding.

bound(d) is the error of the filtered distance against the exact one, as the comment above k_flat_filter_big derives it, in units
of (xn + yn):  dropped products 3.1 * 2^-18, fp32 accumulation of 3 d products 3 d 2^-24 on |x||y| <= (xn + yn) / 2, the fp32
norms d 2^-24, the exact path's own roundings (d / 8 + 4) 2^-24 * 2  --  (3.1 * 2^-18 + (4.25 d + 8) 2^-24) in all, taken on
(xn + yn) whole."""
import numpy as np
import pytest

from gamma_amd import api

TIERS = ((128, 2.0 ** -13), (512, 2.0 ** -12), (1024, 2.0 ** -11), (1536, 2.0 ** -10))      # before any-length rows


def bound(d):
    return 3.1 * 2.0 ** -18 + (4.25 * d + 8) * 2.0 ** -24


MIN_HEADROOM = min(m / bound(d) for d, m in TIERS)


def test_existing_tiers_have_their_smallest_headroom_at_512():
    """the library's constants at the four tier ends are today's, and the floor every new tier is held to comes from them"""
    for lim, m in TIERS:
        assert api.flat_filter_shape(lim) == (lim, m)
        if lim < 1536:
            assert api.flat_filter_shape(lim + 1)[1] == 2 * m      # the next tier starts right behind
    assert MIN_HEADROOM == TIERS[1][1] / bound(512) and 1.7 < MIN_HEADROOM < 1.75
    # (the figures the kernel's comment gives for 1024 and 1536)
    assert abs(bound(1024) - 2.7e-4) < 5e-6 and abs(bound(1536) - 4.0e-4) < 5e-6


def test_every_length_up_to_4096_has_a_shape_and_a_margin():
    last = 0.0
    for d in range(1, 4097):
        shape = api.flat_filter_shape(d)
        assert shape is not None, d
        d_pad, m = shape
        assert d_pad == (d + 31) // 32 * 32
        mant, _ = np.frexp(m)
        assert mant == 0.5, (d, m)                      # a power of two
        assert m >= last, (d, m, last)                  # non-decreasing in d
        last = m
        if d_pad <= 1536:
            assert m == next(t for lim, t in TIERS if d_pad <= lim), (d, m)
        assert m / bound(d_pad) >= MIN_HEADROOM, (d, m, m / bound(d_pad))
    for d in (0, -1, 4097, 1 << 20):
        assert api.flat_filter_shape(d) is None


# ---- the split claim under padding --------------------------------------------------------------------------------------
def _bf16(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u >> 16) & 1) + 0x7FFF
    return ((u + r) & 0xFFFF0000).astype(np.uint32).view(np.float32)


def _split(x):
    hi = _bf16(x)
    return hi, _bf16(x - hi)


def _pad(x, d_pad):
    out = np.zeros((x.shape[0], d_pad), x.dtype)
    out[:, :x.shape[1]] = x
    return out


def _dot(a, b):
    """float64, summed element after element: trailing zeros change nothing, whatever the length"""
    return np.cumsum(a.astype(np.float64) * b.astype(np.float64), axis=1)[:, -1]


def _vectors(kind, n, d, rng):
    if kind == "random":
        return rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((n, d)).astype(np.float32)
    if kind == "wide_range":
        s = (10.0 ** rng.uniform(-3, 3, d)).astype(np.float32)
        return (rng.standard_normal((n, d)).astype(np.float32) * s), (rng.standard_normal((n, d)).astype(np.float32) * s)
    x = (rng.standard_normal((n, d)) * 40).astype(np.float32)      # near-parallel: |x.y| = |x||y| nearly
    return x, (x + rng.standard_normal((n, d)).astype(np.float32) * np.float32(2e-3)).astype(np.float32)


@pytest.mark.parametrize("kind", ["random", "wide_range", "near_parallel"])
@pytest.mark.parametrize("d", [100, 1000, 2500, 4096])
def test_three_products_under_padding(d, kind):
    """x = hi + lo + r; the three products kept miss x.y by at most 3.1 * 2^-18 |x||y|, and zero padding to d_pad changes no sum"""
    d_pad = api.flat_filter_shape(d)[0]
    x, y = _vectors(kind, 64, d, np.random.default_rng(d))
    xh, xl = _split(x)
    yh, yl = _split(y)
    ip = _dot(x, y)
    kept = _dot(xh, yh) + _dot(xh, yl) + _dot(xl, yh)
    nx, ny = np.sqrt(_dot(x, x)), np.sqrt(_dot(y, y))
    rel = np.abs(ip - kept) / (nx * ny)
    print(d, kind, "max |x.y - kept| / |x||y| =", rel.max(), "claim", 3.1 * 2.0 ** -18)
    assert (rel <= 3.1 * 2.0 ** -18).all()
    # the padded vectors: split of a zero is (0, 0), and the sums are the same floats
    xp, yp = _pad(x, d_pad), _pad(y, d_pad)
    xph, xpl = _split(xp)
    yph, ypl = _split(yp)
    assert not xph[:, d:].any() and not xpl[:, d:].any() and not yph[:, d:].any() and not ypl[:, d:].any()
    kept_p = _dot(xph, yph) + _dot(xph, ypl) + _dot(xpl, yph)
    assert np.array_equal(kept, kept_p)
    assert np.array_equal(_dot(xp, xp), _dot(x, x)) and np.array_equal(_dot(yp, yp), _dot(y, y))
