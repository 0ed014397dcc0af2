"""GPU: the filtered re-rank (csrc/rerank_filter.hip) over the shapes rerank_filter_shape_ok admits and tests/test_gpu_rerank_filter.py
does not reach: short-lists of more than one candidate slot per thread (recall_num up to 1024) on real-valued rows, row lengths
from 16 to 1536, ordered batches and the default mode, a call cut into chunks, rows that are not ordinary numbers, an OPQ handle.

Every leg (_leg) checks three things:
  * mode 0 (the plain kernel) and mode 2 (filter forced) answer byte for byte the same, with equal tie_stats (_both);
  * mode 0's answer is the host reference's (tests/rerank_ref.py: the oracle's fvec_L2sqr / fvec_inner_product over the raw rows
    of the candidates GammaHip.last_stages reports) for every query, under compare_topk;
  * rerank_filter_stats: the forced call ran the filter.
Per handle, over its legs: survivors < candidates.  The fraction of survivors is printed per leg -- an observation, no
threshold: with K1 = R (k 63, R 64) nothing can be proven out by construction."""
import numpy as np
import pytest

from gamma_amd import _lib, api
from tests import lloyd
from tests.parity import compare_topk
from tests.rerank_ref import exact_values, topk_of_values
from tests.test_gpu_rerank_filter import M, N, NLIST, NQ, P, WIDE, _both, _rows, _search, _train

pytestmark = pytest.mark.gpu

_cheap = {}


def _data(kind, n, d, seed):
    """"gauss": standard normal; "gauss20": the same scaled and shifted (* 20 + 1000): lo != 0, x - lo cancels"""
    x = _rows("gauss", n, d, seed)
    return x if kind == "gauss" else (x * np.float32(20.0) + np.float32(1000.0)).astype(np.float32)


def _cheap_train(base, nlist, m, centroids_from_rows=False):
    """a codebook whose quality does not matter: two Lloyd iterations (or rows of the base as centroids), three for the PQ"""
    key = (base.shape[1], nlist, m, centroids_from_rows, float(base[0, 0]))
    if key not in _cheap:
        if centroids_from_rows:
            cc = base[np.random.default_rng(7).choice(len(base), nlist, replace=False)].copy()
            _, pq = lloyd.train_ivfpq(base[:3000], 16, m, niter=2, pq_niter=3, seed=1, device="cpu")
        else:
            cc, pq = lloyd.train_ivfpq(base[:3000], nlist, m, niter=2, pq_niter=3, seed=1, device="cpu")
        _cheap[key] = (cc, pq)
    return _cheap[key]


def _build(base, nlist, m, metric, cc, pq, raw=None, opq=None):
    d = base.shape[1]
    g = api.GammaHip(0)
    g.ivfpq_init(d, nlist, m, 8, metric)
    g.ivfpq_set_trained(cc, pq, None)
    if opq is not None:
        g.opq_set(opq)
    g.raw_init(d)
    g.raw_append(base if raw is None else raw)
    g.add(base, 0)
    g.set_small_path(False)
    return g


def _last_recall_ids(g, nq, R):
    """the candidate table of the last chunk of the last call (a call of one chunk: of the call) and the number of its queries"""
    ri = np.full((nq, R), -2, dtype=np.int64)   # (the library writes ids >= -1 into the rows it has)
    g._ck(g.L.gamma_hip_ivfpq_last_stages(g.h, None, None, None, api._p(ri, _lib.i64p)), "last_stages")
    n = int((ri[:, 0] != -2).sum())
    assert n > 0 and (ri[:n] != -2).all() and (ri[n:] == -2).all()
    return ri[:n], n


def _reference(q, raw, ids, k, metric, cache, win):
    """rerank_ref's answer; the exact values of a candidate table are computed once (cache: one table per recall_num)"""
    l2 = metric == api.METRIC_L2
    hit = cache.get(ids.shape[1]) if cache is not None else None
    if hit is None or hit[0] is not raw or not np.array_equal(hit[1], ids):
        hit = (raw, ids.copy()) + exact_values(q, raw, ids, l2)
        if cache is not None:
            cache[ids.shape[1]] = hit
    w = win or WIDE
    return topk_of_values(hit[2], hit[3], ids, k, l2, w["min_score"], w["max_score"]) + (hit[2],)


def _leg(g, q, raw, k, R, metric, what, cache=None, nprobe=P, **win):
    """the three checks of a leg; returns mode 0's (D, I), its tie_stats and the candidates' exact values"""
    nq, Re = len(q), max(R, k)
    s0 = g.rerank_filter_stats()
    D, I, t = _both(g, q, k, R, metric, nprobe=nprobe, **win)
    s1 = g.rerank_filter_stats()
    assert s1["calls"] > s0["calls"] and s1["backoffs"] == s0["backoffs"], (what, s0, s1)
    assert s1["candidates"] - s0["candidates"] == nq * Re
    ids, n = _last_recall_ids(g, nq, Re)
    Dr, Ir, val = _reference(q[nq - n:], raw, ids, k, metric, cache, win)
    compare_topk(Dr, Ir, D[nq - n:], I[nq - n:])
    print("%s R %d k %d: %d of %d candidates survived (%.4f)%s" % (
        what, R, k, s1["survivors"] - s0["survivors"], nq * Re, (s1["survivors"] - s0["survivors"]) / float(nq * Re),
        "" if n == nq else ", reference over the last %d of %d queries" % (n, nq)))
    return D, I, t, val


def _handle_total(g, what):
    st = g.rerank_filter_stats()
    assert st["calls"] >= 1 and 0 < st["survivors"] < st["candidates"], (what, st)
    print("%s, the handle: %d of %d candidates survived (%.4f), %d calls, %d back-offs" % (
        what, st["survivors"], st["candidates"], st["survivors"] / float(st["candidates"]), st["calls"], st["backoffs"]))


# ---- (a) short-lists beyond one candidate slot per thread -----------------------------------------------------------------------
RS_A, KS_A = (64, 65, 255, 256, 257, 512, 513, 1000, 1024), (1, 15, 16, 17, 63)


@pytest.mark.parametrize("metric", [api.METRIC_L2, api.METRIC_IP])
@pytest.mark.parametrize("kind", ["gauss", "gauss20"])
@pytest.mark.parametrize("d", [128, 48])
def test_short_lists_beyond_one_slot_per_thread(d, kind, metric):
    """recall_num around 64 (the head switch of tau with k 15 / 16), around 256 and 512 (a thread's second and third candidate
    slot, the survivors compacted over several ballots) and up to 1024 (the fourth; rerank_first_k over sixteen runs); about
    2 500 candidates per query.  Queries 0 .. 11 are rows, and each of those rows stands 2, 20 or 70 more times in the base
    (inner product: 1.02 times the row, so that the group leads there as well): every k cuts through a group of equal values."""
    base = _data(kind, N, d, 100 + d)
    q = _data(kind, NQ, d, 177 + d)
    q[:12] = base[:12]
    scale = np.float32(1.0 if metric == api.METRIC_L2 else 1.02)
    for i in range(12):
        base[5000 + 100 * i:5000 + 100 * i + (2, 20, 70)[i // 4]] = base[i] * scale
    cc, pq = _train(kind, base, d)
    g = _build(base, NLIST, M, metric, cc, pq)
    what = "(a) d %d %s metric %d" % (d, kind, metric)
    try:
        cache, replayed = {}, 0
        for R in RS_A:
            for k in KS_A:
                D, I, t, val = _leg(g, q, base, k, R, metric, what, cache)
                replayed += t["replayed"]
                assert (I[:12, 0] >= 0).all()
        assert replayed > 0
        # a score window cut through the 1024 candidates, both edges on a candidate's own value
        v = np.sort(val[np.isfinite(val)])
        for k, (a, b) in ((1, (0.3, 0.6)), (16, (0.05, 0.5)), (17, (0.5, 0.95)), (63, (0.4, 0.45))):
            lo, hi = float(v[int(a * len(v))]), float(v[int(b * len(v))])
            Dw, Iw, _, _ = _leg(g, q, base, k, 1024, metric, what + " window", cache, min_score=lo, max_score=hi)
            assert ((Iw < 0) | ((Dw >= np.float32(lo)) & (Dw <= np.float32(hi)))).all() and (Iw >= 0).any()
        _handle_total(g, what)
    finally:
        g.close()


# ---- (b) row lengths ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [api.METRIC_L2, api.METRIC_IP])
@pytest.mark.parametrize("d,m", [(16, 4), (32, 8), (144, 16), (400, 16), (768, 32), (1536, 32)])
def test_row_lengths(d, m, metric):
    """16: one 16-byte piece, seven of a candidate's eight lanes idle; 32: two; 144 and 400: some lanes hold one piece more than
    others; 768; 1536 = kRerankFilterMaxD, all of s_x.  (No coarse stage is compared with anything: beyond 768 the GEMM form is a
    counted deviation, and the re-rank reference does not need it.)"""
    n = 4000 if d == 1536 else 6000
    base = _data("gauss", n, d, 200 + d)
    q = _data("gauss", NQ, d, 277 + d)
    q[:4] = base[:4]
    base[3000:3004] = base[:4]   # ties at the first two ranks
    cc, pq = _cheap_train(base, 16, m)
    g = _build(base, 16, m, metric, cc, pq)
    what = "(b) d %d metric %d" % (d, metric)
    try:
        cache = {}
        for R in (64, 300, 1024):
            for k in (1, 10, 63):
                _leg(g, q, base, k, R, metric, what, cache)
        assert g.rerank_filter_stats()["image_rows"] == n
        _handle_total(g, what)
    finally:
        g.close()


# ---- (c), (d) ordered batches, the default mode, a call cut into chunks ----------------------------------------------------------------
N_C, NLIST_C, P_C = 40000, 1024, 32


def _ordered_case(metric):
    """1024 lists x 16 sub-quantizers x 1 KiB of query table = 16 MiB > 8 MiB: scan_plan.cpp orders the queries of a batch from
    256 on (tests/scan_plan_check.cc holds the rule at this shape), and the re-rank kernel then runs them through qperm"""
    base = _data("gauss", N_C, 128, 300)
    base[20000:20016] = base[:16]   # (queries that are one of these rows find it twice: exact ties)
    cc, pq = _cheap_train(base, NLIST_C, M, centroids_from_rows=True)
    return base, _build(base, NLIST_C, M, metric, cc, pq)


def _plain(g, q, k, args):
    g.tie_stats(reset=True)
    D, I = g.ivfpq_search(q, k, args)
    return D, I, g.tie_stats(reset=True)


@pytest.mark.parametrize("metric", [api.METRIC_L2, api.METRIC_IP])
def test_ordered_batches_and_the_default_mode(metric):
    base, g = _ordered_case(metric)
    what = "(c) metric %d" % metric
    try:
        q = _data("gauss", 1027, 128, 301)
        q[:8] = base[:8]
        # the default mode on a handle whose setter was never called: 1023 queries re-rank plainly, 1027 behind the filter
        default = {}
        for R in (200, 600):
            args = api.SearchArgs(metric=metric, nprobe=P_C, recall_num=R, has_rank=True, exact_ties=1, **WIDE)
            s0 = g.rerank_filter_stats()
            _plain(g, q[:1023], 10, args)
            s1 = g.rerank_filter_stats()
            assert s1["calls"] == s0["calls"] and s1["candidates"] == s0["candidates"]
            D1, I1, t1 = _plain(g, q, 10, args)
            s2 = g.rerank_filter_stats()
            assert s2["calls"] == s1["calls"] + 1 and s2["candidates"] - s1["candidates"] == 1027 * R and s2["image_rows"] == N_C
            ids, n = _last_recall_ids(g, 1027, R)
            assert n == 1027
            Dr, Ir, _ = _reference(q, base, ids, 10, metric, None, None)
            compare_topk(Dr, Ir, D1, I1)
            print("%s 1027 queries, default mode, R %d: %d of %d candidates survived (%.4f)" % (
                what, R, s2["survivors"] - s1["survivors"], 1027 * R, (s2["survivors"] - s1["survivors"]) / (1027.0 * R)))
            default[R] = (D1, I1, t1)
        for R in (200, 600):   # ... and modes 0 and 2 say the same (from here on the setter has been called)
            D0, I0, t0, _ = _leg(g, q, base, 10, R, metric, what + " 1027 queries", nprobe=P_C)
            D1, I1, t1 = default[R]
            assert D0.tobytes() == D1.tobytes() and I0.tobytes() == I1.tobytes() and t0 == t1
        # 300 queries, forced: an ordered batch that is no multiple of 8 -- four workgroups of the rounded grid return early
        for R in (200, 600):
            _leg(g, q[:300], base, 10, R, metric, what + " 300 queries", nprobe=P_C)
        _handle_total(g, what)
    finally:
        g.close()


@pytest.mark.parametrize("metric", [api.METRIC_L2, api.METRIC_IP])
def test_a_call_cut_into_chunks(metric):
    """1027 queries under a workspace budget of about 400 candidate rows: chunks of 400, 400 and 227 queries, the tie replay of
    one chunk beside the next.  last_stages holds the last chunk's tables: that chunk against the reference, all of them by
    mode 0 = mode 2 and by the answer of the uncut call."""
    base, g = _ordered_case(metric)
    what = "(d) metric %d" % metric
    try:
        q = _data("gauss", 1027, 128, 302)
        q[:8] = base[:8]
        q[1019:] = base[8:16]   # queries with ties in the last chunk as well
        whole = {}
        for R in (200, 600):
            whole[R] = _leg(g, q, base, 10, R, metric, what + " uncut", nprobe=P_C)
        # the longest candidate row of the batch decides the chunk (ivfpq_search_device_locked measures it)
        st = g.last_stages(1027, P_C, 600)
        sizes = np.array([g.list_size(l) for l in range(NLIST_C)])
        longest = int(sizes[st["coarse_idx"]].sum(axis=1).max())
        g.set_dist_budget(4 * ((longest + 3) & ~3) * 400)
        flagged = 0
        for R in (200, 600):
            s0 = g.rerank_filter_stats()
            D, I, t, _ = _leg(g, q, base, 10, R, metric, what + " chunked", nprobe=P_C)
            s1 = g.rerank_filter_stats()
            assert s1["calls"] - s0["calls"] >= 2   # one filtered launch per chunk
            _, n = _last_recall_ids(g, 1027, R)
            assert 0 < n < 1027
            assert D.tobytes() == whole[R][0].tobytes() and I.tobytes() == whole[R][1].tobytes()
            flagged += t["replayed"]
        assert flagged > 0
        _handle_total(g, what)
    finally:
        g.close()


# ---- (e) rows that are not ordinary numbers ----------------------------------------------------------------------------------------
BAD = (np.nan, np.inf, -np.inf, 3e38, -3e38, 1e30, 1e-40, -0.0)


def _poke(rows, seed, dim38):
    """one element of every row replaced, the values of BAD in turn; +-3e38 always in dimension dim38 (a span of 6e38 there)"""
    rng = np.random.default_rng(seed)
    rows = rows.copy()
    for i in range(len(rows)):
        v = BAD[i % len(BAD)]
        j = dim38 if abs(v) == 3e38 else int(rng.integers(0, rows.shape[1]))
        if j == dim38 and abs(v) != 3e38:
            j = (j + 1) % rows.shape[1]
        rows[i, j] = np.float32(v)
    return rows


@pytest.mark.parametrize("metric", [api.METRIC_L2, api.METRIC_IP])
@pytest.mark.parametrize("d", [128, 48])
def test_rows_that_are_not_ordinary_numbers(d, metric):
    """The lists index clean vectors; about 1 % of the raw rows -- rows the clean search returns, and more of its candidates --
    carry a NaN, an infinity, +-3e38, 1e30, a denormal or -0.0, so the scan never sees them and the queries stay finite.  A
    candidate whose exact value is NaN or outside the window is never returned, everything else is the reference's.
    First the image is built over such rows: the extrema ignore the non-finite values, the span of 6e38 in one dimension
    overflows and Delta falls back to 1.  (lo = -3e38 in that dimension makes every row's residual overflow: err is infinite,
    every candidate survives -- the answers are what is checked there.)  Then, on an image built over clean rows, such rows
    are appended, written and updated."""
    base = _data("gauss", N, d, 400 + d)
    q = _data("gauss", NQ, d, 477 + d)
    cc, pq = _train("gauss", base, d)
    g = _build(base, NLIST, M, metric, cc, pq)
    what = "(e) d %d metric %d" % (d, metric)
    l2 = metric == api.METRIC_L2
    rng = np.random.default_rng(5)

    def check(D, I, raw):
        val, live = exact_values(q, raw, np.where(I >= 0, I, 0), l2)
        ok = I >= 0
        assert np.isfinite(val[ok]).all() and (np.abs(val[ok]) <= np.float32(3e38)).all()
        assert D[ok].tobytes() == val[ok].tobytes()

    try:
        args = api.SearchArgs(metric=metric, nprobe=P, recall_num=200, has_rank=True, exact_ties=1, **WIDE)
        Dc, Ic, _ = _search(g, 0, q, 10, args)   # (mode 0 builds no image)
        cand, _ = _last_recall_ids(g, NQ, 200)
        assert g.rerank_filter_stats()["image_rows"] == 0
        pool = np.unique(cand[cand >= 0])
        bad = np.unique(np.concatenate([Ic[:, :3].ravel(), rng.choice(pool, 60, replace=False)]))
        bad = bad[bad >= 0]
        assert 150 <= len(bad) <= 260   # about 1 % of the rows
        # -- present when the image is built
        raw = base.copy()
        raw[bad] = _poke(base[bad], 1, dim38=5)
        g.raw_write(0, raw)
        for k in (10, 1):   # (two kinds of call: after a call in which everything survived, the next of its kind backs off)
            D, I, _, _ = _leg(g, q, raw, k, 200, metric, what + " bad rows under the image")
            check(D, I, raw)
            if k == 10:
                assert (I != Ic).any()
        st = g.rerank_filter_stats()
        assert st["image_rows"] == N
        print("%s: image built over the bad rows, %d of %d candidates survived" % (what, st["survivors"], st["candidates"]))
        # -- a new image over clean rows; then the writers bring the bad rows
        g.raw_clear()
        g.raw_append(base)
        raw = base.copy()
        D, I, _, _ = _leg(g, q, raw, 10, 200, metric, what + " clean image")
        assert D.tobytes() == Dc.tobytes() and I.tobytes() == Ic.tobytes() and g.rerank_filter_stats()["image_rows"] == N
        for v, row in zip(bad[:16], _poke(base[bad[:16]], 2, dim38=5)):   # raw_update
            g.raw_update(int(v), row)
            raw[v] = row
        D, I, _, _ = _leg(g, q, raw, 1, 200, metric, what + " raw_update")
        check(D, I, raw)
        first = int(Ic[0, 0]) // 64 * 64   # raw_write: a block of 64 rows around a row that is found, every other one bad
        blk = base[first:first + 64].copy()
        blk[int(Ic[0, 0]) % 2::2] = _poke(blk[int(Ic[0, 0]) % 2::2], 3, dim38=5)
        g.raw_write(first, blk)
        raw[first:first + 64] = blk
        g.raw_update_batch(bad[16:48], _poke(base[bad[16:48]], 4, dim38=5))   # ... and raw_update_batch
        raw[bad[16:48]] = _poke(base[bad[16:48]], 4, dim38=5)
        D, I, _, _ = _leg(g, q, raw, 10, 200, metric, what + " raw_write")
        check(D, I, raw)
        near = (base[Ic[:, 0]] + _data("gauss", NQ, d, 9) * np.float32(0.01)).astype(np.float32)   # raw_append: neighbours of the
        more = np.concatenate([near, near])                                                         # rows found, half of them bad
        more_raw = more.copy()
        more_raw[:NQ] = _poke(near, 6, dim38=5)
        g.raw_append(more_raw)
        g.add(more, N)
        raw = np.concatenate([raw, more_raw])
        for k in (1, 10):
            D, I, _, _ = _leg(g, q, raw, k, 200, metric, what + " raw_append")
            check(D, I, raw)
        assert (I >= N + NQ).any() and g.rerank_filter_stats()["image_rows"] == N + 2 * NQ
        _handle_total(g, what)
    finally:
        g.close()


# ---- (f) OPQ ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [api.METRIC_L2, api.METRIC_IP])
def test_opq_handle(metric):
    """the coarse quantizer, the tables and the scan see the rotated queries; the filter and the exact arithmetic the caller's"""
    d = 128
    base = _data("gauss", N, d, 500)
    q = _data("gauss", NQ, d, 501)
    q[:8] = base[:8]
    base[5000:5008] = base[:8]
    A = np.linalg.qr(np.random.default_rng(11).standard_normal((d, d)))[0].astype(np.float32)
    cc, pq = _train("gauss", base, d)
    g = _build(base, NLIST, M, metric, cc, pq, opq=A)
    what = "(f) OPQ metric %d" % metric
    try:
        assert g.opq_get() is not None
        D, I, t, _ = _leg(g, q, base, 10, 300, metric, what)
        assert t["replayed"] > 0 and (I[:8, 0] >= 0).all()
        _leg(g, q, base, 1, 300, metric, what)
        _handle_total(g, what)
    finally:
        g.close()
