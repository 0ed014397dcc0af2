"""CPU: the two exactness claims the matrix-pipe filter makes for narrow rows (flat_mfma.hip), proven
exhaustively, and the HIPFLAT model's "raw_dtype" key through the host harness.

The filter converts a row to bf16 hi / lo fragments: hi = bf16(x), lo = bf16(x - hi), both round-to-nearest-even.  For rows of
IEEE binary16 the pair is the value itself (11 significant bits fit two bf16 of 8), for byte rows hi alone is; so the margin's
dropped-row term is zero for a narrow store."""

import numpy as np

from gamma_amd import plugin


def bf16_rne(x):
    """fp32 -> bf16 (round to nearest even) -> fp32, for finite x"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return r.astype(np.uint32).view(np.float32)


def test_every_finite_binary16_value_is_its_bf16_hi_plus_lo():
    h = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)
    h = h[np.isfinite(h)]
    assert len(h) == 65536 - 2048           # all but the infinities and NaNs
    x = h.astype(np.float32)
    assert np.array_equal(x.astype(np.float16).view(np.uint16), h.view(np.uint16))     # the widening is exact
    hi = bf16_rne(x)
    d = x - hi                               # exact in fp32 (the filter computes it the same way)
    assert np.array_equal(d.astype(np.float64), x.astype(np.float64) - hi.astype(np.float64))
    lo = bf16_rne(d)
    assert np.array_equal(lo, d)             # nothing is left for a third term
    assert np.array_equal(hi.astype(np.float64) + lo.astype(np.float64), x.astype(np.float64))


def test_every_byte_value_is_one_bf16():
    x = np.arange(-128, 256, dtype=np.float32)
    assert np.array_equal(bf16_rne(x), x)
    assert np.array_equal(bf16_rne(x).view(np.uint32) & 0xFFFF, np.zeros(len(x), np.uint32))


def test_bf16_rne_helper_rounds_to_nearest_even():
    # 1 + 2^-8 is a tie between 1 and 1 + 2^-7: even mantissa wins; 1 + 3 * 2^-8 ties upwards to 1 + 2^-6
    x = np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20], np.float32)
    assert bf16_rne(x).tolist() == [1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7]


def test_hipflat_raw_dtype_key():
    # (loads the host library: a missing one is a failure)
    P = plugin.parse_flat_raw_dtype
    assert P("") == (0, "float32")
    assert P('{"metric_type": "L2"}') == (0, "float32")
    for s, want in (("float32", "float32"), ("float16", "float16"), ("uint8", "uint8"), ("int8", "int8"), ("Float16", "float16"),
                    ("UINT8", "uint8"), ("Int8", "int8"), ("FLOAT32", "float32")):
        assert P('{"metric_type": "L2", "raw_dtype": "%s"}' % s) == (0, want)
    for s in ("uint4", "bfloat16", "half", "", "int16"):
        assert P('{"raw_dtype": "%s"}' % s)[0] != 0
    # the key is HIPFLAT's own: HIPIVFPQ's parser is another function with the same four values
    assert plugin.parse_raw_dtype('{"ncentroids": 16, "nsubvector": 8, "raw_dtype": "int8"}') == (0, "int8")
