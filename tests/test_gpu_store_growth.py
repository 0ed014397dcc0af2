"""GPU: the filter-side arrays (a scalar column, a term column, the vid -> docid map, the delete bitmap) appended in pieces
across their first capacity of 65 536 -- the prefix each reallocation carries over is intact: a handle filled in two pieces
(65 000, then 1 000) answers filtered searches exactly as a handle filled in one call and as the oracle, and between the pieces
exactly as a handle that only ever got the first piece."""
import numpy as np
import pytest

from gamma_amd import api
from oracle import binding as B
from tests import fixtures
from tests.parity import compare_exact

pytestmark = pytest.mark.gpu
WIDE = dict(min_score=-3e38, max_score=3e38)
N, CUT, EDGE = 66000, 65000, 65536
RANGE = (1, 200, 700, True, False)      # column 1 in [200, 700)
TERM = (5, 1, [1, 5])                   # column 5 carries item 1 or item 5


def _fill(case, data, pieces, between=None):
    """a handle that receives vectors, columns, map and delete bits of the vids / docids [lo, hi) of every piece in turn"""
    o = case["oracle"]
    g = api.GammaHip(0)
    g.ivfpq_init(case["d"], case["nlist"], case["M"], 8, case["metric"])
    g.ivfpq_set_trained(case["cc"], case["pq"], None)
    g.raw_init(case["d"])
    lists = [o.get_list(l) for l in range(case["nlist"])]
    for i, (lo, hi) in enumerate(pieces):
        nos, counts, vids, codes = [], [], [], []
        for l, (ids, cds) in enumerate(lists):
            sel = (ids >= lo) & (ids < hi)
            if sel.any():
                nos.append(l), counts.append(int(sel.sum())), vids.append(ids[sel]), codes.append(cds[sel])
        g.add_keys_batch(nos, counts, np.concatenate(vids), np.concatenate(codes))
        g.raw_append(case["base"][lo:hi])
        g.field_append(1, data["price"][lo:hi])
        g.term_append(5, data["items"][lo:hi])
        g.vid2docid_append(data["v2d"][lo:hi])
        g.bitmap_set(data["dead"][(data["dead"] >= lo) & (data["dead"] < hi)])
        if between is not None and i + 1 < len(pieces):
            between(g)
    return g


def test_filter_arrays_keep_their_prefix_across_the_first_growth():
    case = fixtures.trained_case(d=16, nlist=8, M=4, N=N, nq=8)
    rng = np.random.default_rng(65536)
    # two vids per doc for the first 1000 docs, docid == vid behind them (docs 1000 .. 1999 hold no vector)
    v2d = np.arange(N, dtype=np.int32)
    v2d[:2000] = np.arange(2000) // 2
    price = rng.integers(0, 1000, size=N).astype(np.int32)                       # one int value per doc
    items = [rng.integers(0, 12, size=c).tolist() for c in rng.integers(1, 4, size=N)]   # 1 .. 3 items per doc
    dead = np.concatenate([rng.choice(CUT, 50, replace=False), EDGE + rng.choice(N - EDGE, 50, replace=False)]).astype(np.int64)
    data = dict(v2d=v2d, price=price, items=items, dead=dead)
    q = case["q"]

    def admitted(ndocs):
        m = (price[:ndocs] >= RANGE[1]) & (price[:ndocs] < RANGE[2]) & np.array([bool(set(TERM[2]) & set(it)) for it in items[:ndocs]])
        m[dead[dead < ndocs]] = False
        held = np.zeros(ndocs, bool)
        held[v2d[:ndocs]] = True
        return np.nonzero(m & held)[0]

    docs = admitted(N)
    # the filter is the same for every query: it admits docs on both sides of the arrays' first capacity
    assert (docs < EDGE).sum() >= 20 and (docs >= EDGE).sum() >= 20, ((docs < EDGE).sum(), (docs >= EDGE).sum())
    assert (admitted(CUT) < CUT).sum() >= 20
    args = api.SearchArgs(metric=api.METRIC_L2, nprobe=8, recall_num=50, coarse_mode=0, field_filters=[RANGE], term_filters=[TERM], **WIDE)
    mid = {}
    a = _fill(case, data, [(0, CUT), (CUT, N)], between=lambda g: mid.update(r=g.ivfpq_search(q, 10, args)))
    b = _fill(case, data, [(0, N)])
    c = _fill(case, data, [(0, CUT)])
    try:
        Da, Ia = a.ivfpq_search(q, 10, args)
        Db, Ib = b.ivfpq_search(q, 10, args)
        Dc, Ic = c.ivfpq_search(q, 10, args)
        assert Da.tobytes() == Db.tobytes() and np.array_equal(Ia, Ib)                # in pieces == in one call
        assert mid["r"][0].tobytes() == Dc.tobytes() and np.array_equal(mid["r"][1], Ic)   # between the pieces == the first piece alone
        assert (Ia >= 0).all() and np.isin(v2d[Ia], docs).all() and (Ic < CUT).all()
        bm = np.zeros((N >> 3) + 1, dtype=np.uint8)
        np.bitwise_or.at(bm, dead >> 3, (1 << (dead & 7)).astype(np.uint8))
        ctx = B.make_ctx(docids_bitmap=bm, range_filters=[B.make_range_filter(docs)], vid2docid=v2d, **WIDE)
        D, I = case["oracle"].search(q, 10, 8, recall_num=50, has_rank=True, metric=B.METRIC_L2, ctx=ctx, coarse_mode=0)
        compare_exact(D, I, Da, Ia)
        compare_exact(D, I, Db, Ib)
    finally:
        a.close(), b.close(), c.close()
