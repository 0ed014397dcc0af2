"""CPU: the inputs of the GPU tests of the IVFFLAT list shards over float16 / uint8 / int8 rows (tests/ivfflat_shard_rows_data.py,
DESIGN section 33), examined with the oracle before a GPU sees them.  For every case the list-sharded path restated in numpy
(tests/ivfflat_shard_ref.py) over the oracle holding the widened rows W equals the whole-index oracle at every rank; the tie case
of every element type has a query with equal distances from two owners at the k cut and a shard whose own cut went through a
tie, and answers wrongly without the flag rule; the stores' acceptance predicates take every row the tests hand over.

The seeds of the tie cases were picked on the CPU and are fixed (ivfflat_shard_rows_data.TIE_SEED)."""
import numpy as np
import pytest

from tests import ivfflat_rows_data as R
from tests import ivfflat_shard_ref as SR
from tests import ivfflat_shard_rows_data as RD
from tests.parity import compare_exact

K, P = RD.K, RD.P


@pytest.mark.parametrize("dtype", RD.DTYPES)
@pytest.mark.parametrize("d,metric,W", RD.SHAPES)
def test_sharded_path_equals_the_whole_index(d, metric, W, dtype):
    c = RD.case(d, dtype, metric)
    assert c.raw.tobytes() == c.W.tobytes()      # the oracle holds the widened rows
    if dtype == "float16":
        assert (c.W != c.base).mean() > 0.9
    else:
        assert np.array_equal(c.W, c.base)
    assert RD.storable(c.base, dtype)
    owner = SR.owners_mod(c.nlist, W)
    D0, I0 = c.oracle(c.q, K, P, **SR.WIDE)
    D, I, _ = SR.sharded_search(c, c.q, K, P, W, owner, **SR.WIDE)
    compare_exact(D0, I0, D, I)
    # the two sides of the 2 nlist threshold and k beyond the candidates, as the GPU test runs them
    D0, I0 = c.oracle(c.q[:7], K, P, **SR.WIDE)
    D, I, _ = SR.sharded_search(c, c.q[:7], K, P, W, owner, **SR.WIDE)
    compare_exact(D0, I0, D, I)
    assert 33 * P >= 2 * c.nlist > 7 * P
    D0, I0 = c.oracle(c.q, 500, 2, **SR.WIDE)
    D, I, _ = SR.sharded_search(c, c.q, 500, 2, W, owner, **SR.WIDE)
    assert (I0 == -1).any()
    compare_exact(D0, I0, D, I)


@pytest.mark.parametrize("dtype", RD.DTYPES)
@pytest.mark.parametrize("metric,W", RD.TIE_SHAPES)
def test_tie_cases_exercise_the_flag_rule(metric, W, dtype):
    c = RD.tie_case(dtype, metric)
    lo, hi = (-128, 127) if dtype == "int8" else (0, 255)
    assert c.base.min() >= lo and c.base.max() <= hi and np.array_equal(c.base, np.rint(c.base))
    assert np.array_equal(R.widened(c.base, dtype), c.base) and RD.storable(c.base, dtype)      # exact in the type
    owner = SR.owners_mod(c.nlist, W)
    D0, I0 = c.oracle(c.q, K, P, **SR.WIDE)
    D, I, info = SR.sharded_search(c, c.q, K, P, W, owner, **SR.WIDE)
    assert info["cross"].any(), "no query with equal distances from two owners at the k cut"
    assert info["shard_cut"].any(), "no shard whose own cut went through a tie"
    assert info["flagged"].sum() > 0
    compare_exact(D0, I0, D, I)
    Dn, In, _ = SR.sharded_search(c, c.q, K, P, W, owner, rule="never", **SR.WIDE)
    with pytest.raises(AssertionError):
        compare_exact(D0, I0, Dn, In)


def test_the_chunked_tie_case_is_the_l2_two_owner_one():
    c = RD.tie_case("uint8", RD.L2)
    _, _, info = SR.sharded_search(c, c.q, K, P, 2, SR.owners_mod(c.nlist, 2), **SR.WIDE)
    assert info["shard_cut"].any() and info["flagged"].sum() > 0


@pytest.mark.parametrize("dtype", RD.DTYPES)
def test_edge_update_and_filter_cases(dtype):
    from tests import ivfflat_lm_data as LM
    c = RD.edge_case(dtype)
    assert [len(c.lists[l]) for l in (LM.EDGE_128, LM.EDGE_129, LM.EDGE_EMPTY)] == [128, 129, 0]
    cnt = LM.probes_per_list(c, c.q, P)
    assert cnt[LM.EDGE_128] > 0 and cnt[LM.EDGE_129] > 0 and cnt[LM.EDGE_EMPTY] > 0 and cnt[LM.EDGE_129] < len(c.q)
    owner = np.zeros(c.nlist, dtype=np.int64)
    owner[LM.EDGE_129] = 1
    owner[LM.EDGE_EMPTY] = 2
    D0, I0 = c.oracle(c.q, K, P, **SR.WIDE)
    D, I, _ = SR.sharded_search(c, c.q, K, P, 3, owner, **SR.WIDE)
    compare_exact(D0, I0, D, I)
    assert RD.storable(c.base, dtype)
    # the row the update test writes is one the store takes, and (float16) one the store changes
    cu = RD.edge_case(dtype, seed=RD.UPDATE_SEED)
    new, held = RD.changed_row(cu, dtype, int(cu.lists[LM.EDGE_129][0]))
    assert RD.storable(new[None], dtype)
    assert (held != new).any() == (dtype == "float16")
    assert RD.storable(RD.filter_case(dtype).base, dtype)


def test_the_predicates_refuse_what_the_gpu_tests_call_unstorable():
    x = np.zeros((2, 16), np.float32)
    for dtype, v in (("float16", 1e6), ("uint8", 0.5), ("int8", 200.0)):
        assert RD.storable(x, dtype)
        y = x.copy()
        y[1, 7] = v
        assert not RD.storable(y, dtype)
