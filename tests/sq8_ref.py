"""The arithmetic of the scalar-quantised raw store (include/gamma_hip.h, gamma_hip_raw_init_sq8) restated in numpy: every step
is one elementwise fp32 operation, so numpy gives the same bits as the host's derivation, the device's encoder and the
re-rank kernels' decode.  The yardstick of the sq8 tests."""
import numpy as np

F = np.float32


def params(vmin, vmax):
    """(step, inv) of the ranges; ValueError for what gamma_hip_raw_sq8_params refuses"""
    vmin, vmax = np.asarray(vmin, F), np.asarray(vmax, F)
    with np.errstate(all="ignore"):
        span = vmax - vmin
        if not (np.isfinite(vmin).all() and np.isfinite(vmax).all() and (vmin <= vmax).all() and np.isfinite(span).all()):
            raise ValueError("refused ranges")
        step = span / F(255.0)
        inv = F(255.0) / span
    const = (span == 0) | ~np.isfinite(inv)
    return np.where(const, F(0), step).astype(F), np.where(const, F(0), inv).astype(F)


def encode(x, vmin, inv):
    """a subtract, a multiply, a round-half-to-even and a clamp, each rounded in fp32; a constant dimension: code 0"""
    x, vmin, inv = np.asarray(x, F), np.asarray(vmin, F), np.asarray(inv, F)
    with np.errstate(all="ignore"):
        r = np.rint((x - vmin) * inv)
        c = np.minimum(np.maximum(r, F(0.0)), F(255.0))
    return np.where(np.broadcast_to(inv == 0, c.shape), F(0), c).astype(np.uint8)


def decode(c, vmin, step):
    """a multiply, then an add, each rounded in fp32"""
    t = np.asarray(c).astype(F) * np.asarray(step, F)
    return (np.asarray(vmin, F) + t).astype(F)


def stored(x, vmin, vmax):
    """W = decode(encode(x)): the rows an sq8 store with these ranges holds for x"""
    step, inv = params(vmin, vmax)
    return decode(encode(x, vmin, inv), vmin, step)


def rows(n, d, seed, wide=1.0):
    """Gaussian fp32 rows with a scale and an offset of their own per dimension (fixed per d): magnitudes over three decades,
    every third dimension negative throughout, and for d > 1 one dimension constant at 0.75 while wide == 1 (wider rows vary
    it, and reach beyond ranges trained on rows of wide == 1 at both ends)"""
    p = np.random.default_rng(1000 + d)
    scale = 10.0 ** p.uniform(-2.0, 1.0, d)
    offset = p.uniform(-3.0, 3.0, d) * scale
    offset[::3] = -8.0 * scale[::3]
    x = offset + scale * wide * np.random.default_rng(seed).standard_normal((n, d))
    if d > 1:
        cd = min(5, d - 1)
        x[:, cd] = 0.75 if wide == 1.0 else 0.75 + 0.1 * np.random.default_rng(seed + 1).standard_normal(n)
    return np.ascontiguousarray(x, dtype=F)
