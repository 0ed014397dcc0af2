"""A host reference of the exact re-rank stage (ivfpq_stage_b over a dense fp32 raw store: k_rerank_topk, k_rerank_topk_filt).

rerank_reference takes what the stage takes -- the caller's queries, the raw rows as the store holds them, the candidate table
of the recall stage -- and answers what it has to answer, without a device:
  * a candidate's exact value is the oracle's go_fvec_L2sqr / go_fvec_inner_product (pinned against the compiled library) of
    the query and the candidate's raw row;
  * a candidate is dropped when its id is -1 or at / beyond the row count, when its value is NaN, or when the value lies
    outside [min_score, max_score];
  * the first k by value (L2 ascending, inner product descending), then (neutral, -1) padding as rerank_topk_out writes it.
Compare with tests/parity.py::compare_topk: the order inside a group of equal values is the reference heaps' and not this
module's.

exact_chain is the same arithmetic written out in numpy (the eight lane accumulators of rerank_dev.h); the CPU test of the
filter's bound holds lb / ub against it."""
import numpy as np

F = np.float32
NEUTRAL = {True: F(3.402823466e+38), False: F(-3.402823466e+38)}   # (L2, inner product): neutral_of, gamma_hip_search.h


def fma32(a, b, c):
    """fp32 fma: the product of two floats is exact in float64"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def exact_chain(x, y, l2):
    """x[nq, d], y[ny, d] -> [nq, ny]: the reference's chain.  Lane l runs elements l, l + 8, ..; s[l] = acc[l + 4] + acc[l];
    (s0 + s1) + (s2 + s3).  d % 8 == 0."""
    d = x.shape[-1]
    assert d % 8 == 0
    acc = np.zeros((x.shape[0], y.shape[0], 8), F)
    for i in range(0, d, 8):
        xs, ys = x[:, None, i:i + 8], y[None, :, i:i + 8]
        if l2:
            t = (xs - ys).astype(F)
            acc = fma32(t, t, acc)
        else:
            acc = fma32(np.broadcast_to(xs, acc.shape), np.broadcast_to(ys, acc.shape), acc)
    s = acc[..., 4:] + acc[..., :4]
    return (s[..., 0] + s[..., 1]) + (s[..., 2] + s[..., 3])


def exact_values(q, raw, ids, l2):
    """[nq, R] oracle values of query i against the rows ids[i]; NaN where the id names no row"""
    from oracle import binding as B
    L = B.lib()
    q = np.ascontiguousarray(q, dtype=F)
    raw = np.ascontiguousarray(raw, dtype=F)
    nq, R = ids.shape
    n, d = raw.shape
    assert q.shape == (nq, d) and d >= 16   # (below 16 the _ny entries are forms of their own, not the per-row function)
    fn = L.go_fvec_L2sqr_ny if l2 else L.go_fvec_inner_products_ny
    live = (ids >= 0) & (ids < n)
    val = np.empty((nq, R), F)
    for i in range(nq):
        rows = np.ascontiguousarray(raw[np.where(live[i], ids[i], 0)])
        out = np.empty(R, F)
        fn(B._fp(out), B._fp(q[i]), B._fp(rows), d, R)
        val[i] = out
    val[~live] = np.nan
    return val, live


def topk_of_values(val, live, ids, k, l2, min_score, max_score):
    """the first k usable candidates by value, padded"""
    nq, R = val.shape
    lo, hi = F(min_score), F(max_score)
    with np.errstate(invalid="ignore"):
        ok = live & (val <= hi) & (val >= lo)   # (false for NaN)
    key = np.where(ok, val if l2 else -val, F(np.inf)).astype(F)
    order = np.argsort(key, axis=1, kind="stable")[:, :k]
    D = np.full((nq, k), NEUTRAL[bool(l2)], F)
    I = np.full((nq, k), -1, np.int64)
    kk = order.shape[1]
    took = np.take_along_axis(ok, order, axis=1)
    D[:, :kk] = np.where(took, np.take_along_axis(val, order, axis=1), D[:, :kk])
    I[:, :kk] = np.where(took, np.take_along_axis(ids, order, axis=1), -1)
    return D, I


def rerank_reference(q, raw, recall_ids, k, l2, min_score, max_score):
    """(D[nq, k], I[nq, k]) of the re-rank stage; l2: the metric (True: L2, False: inner product)"""
    ids = np.ascontiguousarray(recall_ids, dtype=np.int64)
    val, live = exact_values(q, raw, ids, l2)
    return topk_of_values(val, live, ids, k, l2, min_score, max_score)
