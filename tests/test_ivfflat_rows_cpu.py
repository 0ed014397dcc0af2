"""CPU: the HIPIVFFLAT model's "raw_dtype" key through the host harness, and the properties of the test data that the GPU tests
of IVFFLAT over narrow rows (tests/test_gpu_ivfflat_rows.py) rely on -- examined here with the oracle, so that
those tests cannot pass vacuously."""
import numpy as np
import pytest

from gamma_amd import plugin
from oracle import binding as B
from tests import ivfflat_rows_data as R


def test_hipivfflat_raw_dtype_key():
    # (loads the host library: a missing one is a failure)
    P = plugin.parse_ivfflat_raw_dtype
    assert P("") == (0, "float32")
    assert P('{"ncentroids": 16, "metric_type": "L2"}') == (0, "float32")
    for s, want in (("float32", "float32"), ("float16", "float16"), ("uint8", "uint8"), ("int8", "int8"), ("Float16", "float16"),
                    ("UINT8", "uint8"), ("Int8", "int8"), ("FLOAT32", "float32")):
        assert P('{"ncentroids": 16, "raw_dtype": "%s"}' % s) == (0, want)
    for s in ("uint4", "bfloat16", "half", "", "int16"):
        assert P('{"raw_dtype": "%s"}' % s)[0] != 0


def test_float16_rows_differ_from_their_fp32_source():
    """rounding to half must change the data, or a reader that took the caller's fp32 would pass too"""
    base = R.base_rows(3001, 32, "float16", 100)
    W = R.widened(base, "float16")
    assert (W != base).mean() > 0.9
    assert np.array_equal(R.widened(W, "float16"), W)       # W is what a float16 store holds exactly
    q = R.queries(8, 32, "float16", 300, W)
    D0, _ = B.flat_search(base, q, 10, B.METRIC_L2, B.make_ctx())
    D1, _ = B.flat_search(W, q, 10, B.METRIC_L2, B.make_ctx())
    assert D0.tobytes() != D1.tobytes()                      # ... and the difference reaches the results


@pytest.mark.parametrize("dtype", ["uint8", "int8"])
def test_byte_rows_are_inside_their_type(dtype):
    base = R.base_rows(3001, 32, dtype, 100)
    lo, hi = R.RANGE[dtype]
    assert base.min() == lo and base.max() == hi and np.array_equal(base, np.rint(base))
    assert np.array_equal(R.widened(base, dtype), base)


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("metric", [B.METRIC_L2, B.METRIC_IP], ids=["l2", "ip"])
def test_tie_data_has_a_tie_at_the_k_cut(dtype, metric):
    """under the oracle's IVFFLAT search over the lists the GPU test uses: rank k - 1 and rank k hold the same distance and
    different rows for every query"""
    c = R.Case(64, dtype, metric, ties=True, seed=7)
    D, I = c.oracle(c.q, R.TIE_K + 1, 4)
    assert (I >= 0).all()
    assert (D[:, R.TIE_K - 1] == D[:, R.TIE_K]).all() and (I[:, R.TIE_K - 1] != I[:, R.TIE_K]).all()


def test_the_empty_list_case_has_an_empty_list_that_queries_probe():
    c = R.Case(32, "uint8", B.METRIC_L2, empty=5, seed=3)
    assert len(c.lists[5]) == 0 and sum(len(l) for l in c.lists) == c.N
    _, _, st = B.ivfflat_search(c.o, c.q, 10, 4, B.METRIC_L2, B.make_ctx(), want_stages=True)
    assert (st["coarse_idx"] == 5).any()
    # lists of about 190 rows: two 128-row chunks with a partial one
    assert max(len(l) for l in c.lists) > 128
