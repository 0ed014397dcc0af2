"""CPU: the list-sharded IVFFLAT path restated in numpy (tests/ivfflat_shard_ref.py) equals the oracle's IVFFLAT search on the
whole index -- labels at every rank, exact ties included -- for 2, 3 and 4 owners, L2 and inner product, and the data exercise
the flag rule: at least one query has equal distances from lists of two different owners at the k cut, at least one has a
shard whose own cut went through a tie, and with the rule weakened to "never flag" the same comparison fails.

The seed of the tie case was picked on the CPU (seeds 0 .. 5 all serve; 3 gives both properties for every W and both owner
maps) and is fixed."""
import numpy as np
import pytest

from oracle import binding as B
from tests import ivfflat_lm_data as LM
from tests import ivfflat_shard_ref as SR
from tests.parity import compare_exact

L2, IP = B.METRIC_L2, B.METRIC_IP
SEED, K, P = 3, 10, 4

_cases = {}


def tie_case(metric):
    if metric not in _cases:
        c = SR.TieCase(metric=metric, seed=SEED)
        _cases[metric] = (c, c.oracle(c.q, K, P, **SR.WIDE))
    return _cases[metric]


def owners(c, W, how):
    return SR.owners_mod(c.nlist, W) if how == "mod" else SR.owners_by_size(c.lists, W)


@pytest.mark.parametrize("how", ["mod", "size"])
@pytest.mark.parametrize("W", [2, 3, 4])
@pytest.mark.parametrize("metric", [L2, IP], ids=["l2", "ip"])
def test_sharded_path_equals_the_whole_index_on_tie_data(metric, W, how):
    c, (D0, I0) = tie_case(metric)
    owner = owners(c, W, how)
    assert len(set(owner.tolist())) == W
    D, I, info = SR.sharded_search(c, c.q, K, P, W, owner)
    # the data do their job
    assert info["cross"].any(), "no query with equal distances from two owners at the k cut"
    assert info["shard_cut"].any(), "no shard whose own cut went through a tie"
    compare_exact(D0, I0, D, I)
    # ... and the rule is what makes it so: without any flag the merged top-k is NOT the whole index's answer
    Dn, In, _ = SR.sharded_search(c, c.q, K, P, W, owner, rule="never")
    with pytest.raises(AssertionError):
        compare_exact(D0, I0, Dn, In)


@pytest.mark.parametrize("W", [2, 3, 4])
@pytest.mark.parametrize("metric", [L2, IP], ids=["l2", "ip"])
def test_sharded_path_on_rows_without_ties(metric, W):
    """fp32 rows: (almost) no query is flagged, the merge alone answers"""
    c = LM.Case(24, "float32", metric, seed=40 + W)
    D0, I0 = c.oracle(c.q, K, P, **SR.WIDE)
    D, I, info = SR.sharded_search(c, c.q, K, P, W, SR.owners_mod(c.nlist, W))
    assert not info["flagged"].all()
    compare_exact(D0, I0, D, I)


def test_k_beyond_the_candidates_and_a_shard_without_probed_lists():
    c = LM.Case(24, "float32", L2, N=300, seed=47)
    owner = np.zeros(c.nlist, dtype=np.int64)
    owner[5] = 1      # member 1 owns one list: most queries probe none of its lists
    k = 200           # more than the probed lists hold
    D0, I0, st = B.ivfflat_search(c.o, c.q, k, 2, c.metric, B.make_ctx(**SR.WIDE), want_stages=True)
    assert (I0 == -1).any() and not (st["coarse_idx"] == 5).any(axis=1).all()
    D, I, _ = SR.sharded_search(c, c.q, k, 2, 2, owner)
    compare_exact(D0, I0, D, I)
