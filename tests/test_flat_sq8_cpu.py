"""CPU: HIPFLAT's "raw_dtype": "sq8" with its two keys through the harness (gamma_amd/host, no GPU), and the precondition under
which the matrix filter's margin -- proven for finite fp32 rows -- covers a decoded sq8 row: every decoded value is finite."""
import numpy as np

from gamma_amd import plugin
from tests import sq8_ref as S

REJECTED = (-1, "float32")


def test_hipflat_sq8_keys():
    # (loads the host library: a missing one is a failure)
    P = plugin.parse_flat_raw_dtype
    for s in ('{"raw_dtype": "sq8", "sq8_min": -1.5, "sq8_max": 2}',
              '{"metric_type": "InnerProduct", "raw_dtype": "SQ8", "sq8_min": -0.25, "sq8_max": 0.25, "exact_ties": 1}',
              '{"raw_dtype": "Sq8", "sq8_min": 0, "sq8_max": 0}',                    # a constant range: step 0
              '{"raw_dtype": "sq8", "sq8_min": -1e38, "sq8_max": 1e38}',             # the span is finite as a float
              '{"raw_dtype": "sq8", "sq8_min": 1e-45, "sq8_max": 3}'):
        assert P(s) == (0, "sq8"), s
    for s in ('{"metric_type": "L2", "raw_dtype": "sq8"}',                            # both keys are required
              '{"raw_dtype": "sq8", "sq8_min": 0}',
              '{"raw_dtype": "sq8", "sq8_max": 1}',
              '{"raw_dtype": "sq8", "sq8_min": "0", "sq8_max": 1}',                  # as numbers
              '{"raw_dtype": "sq8", "sq8_min": [0], "sq8_max": 1}',
              '{"raw_dtype": "sq8", "sq8_min": null, "sq8_max": 1}',
              '{"raw_dtype": "sq8", "sq8_min": 2, "sq8_max": 1}',                    # sq8_min > sq8_max
              '{"raw_dtype": "sq8", "sq8_min": 0, "sq8_max": 1e39}',                 # not finite as a float
              '{"raw_dtype": "sq8", "sq8_min": -1e39, "sq8_max": 0}',
              '{"raw_dtype": "sq8", "sq8_min": nan, "sq8_max": 1}',
              '{"raw_dtype": "sq8", "sq8_min": 0, "sq8_max": inf}',
              '{"raw_dtype": "sq8", "sq8_min": -3e38, "sq8_max": 3e38}',             # the span is not (the store refuses it)
              '{"raw_dtype": "uint8", "sq8_min": 0, "sq8_max": 1}',                  # either key with another raw_dtype
              '{"raw_dtype": "float32", "sq8_max": 1}',
              '{"metric_type": "L2", "sq8_min": 0}',
              '{"raw_dtype": "sq4", "sq8_min": 0, "sq8_max": 1}',
              '{"raw_dtype": "sq8", "sq8_min": 0, "sq8_max": 1'):                    # does not parse
        assert P(s) == REJECTED, s
    # the other values answer as before, and HIPIVFFLAT keeps rejecting sq8 with or without the keys
    assert P("") == (0, "float32") and P('{"raw_dtype": "Int8"}') == (0, "int8")
    assert plugin.parse_ivfflat_raw_dtype('{"ncentroids": 16, "raw_dtype": "sq8", "sq8_min": 0, "sq8_max": 1}')[0] == -1


def test_every_decoded_value_is_finite():
    """200 random ranges the store accepts (gamma_hip_raw_sq8_params: finite bounds, vmin <= vmax, a finite span) over 38 decades
    and both signs, the extremes of fp32 and constant ranges among them: all 256 codes decode to a finite fp32 value inside
    [vmin, vmax] up to one rounding of the span.  That is what lets the matrix filter treat a decoded row as any fp32 row."""
    rng = np.random.default_rng(20)
    mag = (10.0 ** rng.uniform(-38, 38, (200, 2))) * rng.choice([-1.0, 1.0], (200, 2))
    lo, hi = np.minimum(mag[:, 0], mag[:, 1]).astype(np.float32), np.maximum(mag[:, 0], mag[:, 1]).astype(np.float32)
    fmax = np.finfo(np.float32).max
    lo[:6] = [-fmax / 2, 0.0, -fmax, 1.5, -1e-45, fmax / 2]
    hi[:6] = [fmax / 2, fmax, 0.0, 1.5, 1e-45, fmax]
    step, inv = S.params(lo, hi)                       # (raises for a range the store refuses)
    codes = np.arange(256, dtype=np.uint8)[:, None]
    W = S.decode(codes, lo[None, :], step[None, :])
    assert W.dtype == np.float32 and W.shape == (256, 200) and np.isfinite(W).all()
    span = hi.astype(np.float64) - lo.astype(np.float64)
    slack = np.abs(span) * 2.0 ** -22 + 1e-45
    assert (W >= lo - slack).all() and (W <= hi + slack).all()
    assert (W[:, step == 0] == lo[step == 0]).all() and (step == 0).sum() >= 1
