"""CPU: the HIPIVFFLAT model's "raw_dtype": "sq8" key through the host harness, and the properties of the test data that the GPU
tests of IVFFLAT over sq8 rows (tests/test_gpu_ivfflat_sq8.py) rely on -- examined here with the oracle, so
that those tests cannot pass vacuously."""
import numpy as np
import pytest

from gamma_amd import plugin
from oracle import binding as B
from tests import ivfflat_sq8_data as Q
from tests import sq8_ref as S


def test_hipivfflat_sq8_key():
    # (loads the host library: a missing one is a failure)
    P = plugin.parse_ivfflat_raw_dtype
    # the three rejections that were there before stay
    assert P('{"ncentroids": 16, "raw_dtype": "sq8"}') == (-1, "float32")
    assert P('{"raw_dtype": "SQ8"}') == (-1, "float32")
    assert P('{"raw_dtype": "sq8", "sq8_min": -1.0, "sq8_max": 1.0}') == (-1, "float32")
    # the accepted form: the value together with the key that says where the ranges come from, both case-insensitive
    for rdt, rng in (("sq8", "trained"), ("SQ8", "Trained"), ("Sq8", "TRAINED")):
        assert P('{"ncentroids": 16, "metric_type": "L2", "raw_dtype": "%s", "sq8_ranges": "%s"}' % (rdt, rng)) == (0, "sq8")
    # any other value of the key, a value that is no string
    for rng in ('"given"', '""', '"train"', "1", "true"):
        assert P('{"raw_dtype": "sq8", "sq8_ranges": %s}' % rng) == (-1, "float32")
    # the key beside another raw_dtype, or beside none
    for rdt in ("float32", "float16", "uint8", "int8"):
        assert P('{"raw_dtype": "%s", "sq8_ranges": "trained"}' % rdt) == (-1, "float32")
    assert P('{"ncentroids": 16, "sq8_ranges": "trained"}') == (-1, "float32")
    # HIPFLAT's keys: this model's ranges are trained
    assert P('{"raw_dtype": "sq8", "sq8_ranges": "trained", "sq8_min": -1.0, "sq8_max": 1.0}') == (-1, "float32")
    assert P('{"raw_dtype": "sq8", "sq8_ranges": "trained", "sq8_max": 1.0}') == (-1, "float32")
    # everything else answers as before
    assert P("") == (0, "float32")
    assert P('{"ncentroids": 16, "raw_dtype": "uint8"}') == (0, "uint8")
    assert P('{"raw_dtype": "uint4"}')[0] != 0
    # the two other models' parsers are where they were
    assert plugin.parse_flat_raw_dtype('{"raw_dtype": "sq8", "sq8_ranges": "trained"}') == (-1, "float32")
    assert plugin.parse_raw_dtype('{"ncentroids": 16, "nsubvector": 8, "raw_dtype": "sq8"}') == (0, "sq8")


@pytest.mark.parametrize("d", [32, 144])
def test_the_store_is_lossy_clips_and_has_a_constant_dimension(d):
    """W != base, codes 0 and 255 occur in the half the ranges did not see, one step is 0 -- and the difference between W and
    base reaches the oracle's IVFFLAT results, so a reader of the caller's fp32 rows would not pass"""
    c = Q.Case(d, B.METRIC_L2, seed=d)
    step, inv = S.params(c.vmin, c.vmax)
    codes = S.encode(c.base[c.N // 2:], c.vmin, inv)
    assert (codes == 0).any() and (codes == 255).any() and (step == 0).sum() == 1
    assert (c.W != c.base).mean() > 0.9 and np.isfinite(c.W).all()
    assert np.array_equal(c.stored(c.W), c.W)      # W is what the store holds exactly
    D1, I1 = c.oracle(c.q, 10, 4)
    c.o.set_raw(c.base)
    D0, I0 = c.oracle(c.q, 10, 4)
    differs = (D0 != D1).any(axis=1)
    assert differs.any() and (I1 >= 0).all()
    # lists of about 190 rows: one full 128-row chunk and a partial one
    assert max(len(l) for l in c.lists) > 128 and sum(len(l) for l in c.lists) == c.N


@pytest.mark.parametrize("metric", [B.METRIC_L2, B.METRIC_IP], ids=["l2", "ip"])
@pytest.mark.parametrize("d,nq", [(64, 33), (144, 33), (64, 7), (100, 40)])
def test_tie_data_has_a_tie_at_the_k_cut(d, nq, metric):
    """under the oracle's IVFFLAT search over the lists the GPU test uses (its four cases): rank k - 1 and rank k hold the same
    distance and different rows for every query"""
    c = Q.Case(d, metric, nq=nq, ties=True, seed=7)
    D, I = c.oracle(c.q, Q.TIE_K + 1, 4)
    assert (I >= 0).all()
    assert (D[:, Q.TIE_K - 1] == D[:, Q.TIE_K]).all() and (I[:, Q.TIE_K - 1] != I[:, Q.TIE_K]).all()


def test_the_empty_list_case_has_an_empty_list_that_queries_probe():
    c = Q.Case(32, B.METRIC_L2, empty=5, seed=3)
    assert len(c.lists[5]) == 0 and sum(len(l) for l in c.lists) == c.N
    assert Q.probes_per_list(c, c.q, 4)[5] > 0
    assert max(len(l) for l in c.lists) > 128


def test_the_edge_case_has_lists_of_128_and_129_rows_that_queries_probe():
    c = Q.edge_case()
    assert [len(c.lists[l]) for l in (Q.EDGE_128, Q.EDGE_129, Q.EDGE_EMPTY)] == [128, 129, 0]
    cnt = Q.probes_per_list(c, c.q, 4)
    assert cnt[Q.EDGE_128] > 0 and cnt[Q.EDGE_129] > 0 and cnt[Q.EDGE_EMPTY] > 0


def test_a_list_probed_by_more_queries_than_either_tile():
    """33 queries x 16 probes of 16 lists: every list is probed by 33 queries, a second tile of the fixed-length kernel (32
    queries per tile) and a third of the row-sliced one (16)"""
    c = Q.Case(48, B.METRIC_L2, seed=48)
    assert (Q.probes_per_list(c, c.q, 16) == 33).all()
