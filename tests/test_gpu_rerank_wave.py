"""GPU: the wave-per-query form of the filtered re-rank (k_rerank_topk_filt_wave, csrc/rerank_filter.hip) against the workgroup
kernel and the plain one.

Every case (_four) runs four searches on ONE handle -- filter off; filter forced with form 1 (workgroup kernel always), form 2
(wave form wherever rerank_filter_wave_ok admits the shape: d 128, R <= 256, min(k + 1, R) <= 64) and form 0 (automatic: the
wave form where it is admitted and the call has at least rerank_filter_form()["auto_min_nq"] queries) -- and
asserts that the four (D, I) are byte-identical, that tie_stats are equal, and, from rerank_filter_form, that the kernel each
forced call ran is the one its form and shape ask for.

Handles as in tests/test_gpu_rerank_filter.py: 20 000 rows, 64 lists, M 16, d 128, small path off, exact ties on, so that any
query count reaches the fused re-rank.  The grids use 7 queries: three calls of one kind then stay below the 4096 candidates at
which the handle's feedback decides, so no call is turned down where K1 = R lets every candidate survive."""
import threading

import numpy as np
import pytest

from gamma_amd import api
from tests.rerank_ref import exact_values
from tests.test_gpu_rerank_filter import N, NLIST, NQ, P, WIDE, _handle, _rows, _search
from tests.test_gpu_rerank_filter_shapes import P_C, _data, _last_recall_ids, _ordered_case

pytestmark = pytest.mark.gpu

WG, WAVE = 1, 2


def _wave_ok(d, R, k):
    return d == 128 and 1 <= R <= 256 and min(k + 1, R) <= 64


def _four(g, q, k, R, metric, nprobe=P, d=128, **win):
    """the four searches; returns mode 0's (D, I, tie_stats) and the survivors the three filtered calls counted"""
    args = api.SearchArgs(metric=metric, nprobe=nprobe, recall_num=R, has_rank=True, exact_ties=1, **(win or WIDE))
    Re = max(R, k)
    g.set_rerank_filter_form(0)
    D0, I0, t0 = _search(g, 0, q, k, args)
    surv = 0
    for form in (1, 2, 0):
        g.set_rerank_filter_form(form)
        assert g.rerank_filter_form()["form"] == form
        s0, w0 = g.rerank_filter_stats(), g.rerank_filter_form()["wave_calls"]
        D, I, t = _search(g, 2, q, k, args)
        s1, f = g.rerank_filter_stats(), g.rerank_filter_form()
        assert D.tobytes() == D0.tobytes() and I.tobytes() == I0.tobytes(), (form, k, R, len(q))
        assert t == t0, (form, t0, t)
        assert s1["calls"] == s0["calls"] + 1 and s1["backoffs"] == s0["backoffs"], (form, k, R, s0, s1)
        assert s1["candidates"] - s0["candidates"] == len(q) * Re
        want = WAVE if _wave_ok(d, Re, k) and (form == 2 or (form == 0 and len(q) >= f["auto_min_nq"])) else WG
        assert f["last"] == want and f["wave_calls"] - w0 == (1 if want == WAVE else 0), (form, k, R, f)
        surv += s1["survivors"] - s0["survivors"]
    g.set_rerank_filter_form(0)
    return D0, I0, t0, surv


def _tied(base, q, metric, n=4):
    """queries 0 .. n - 1 are rows, and each of those rows stands twice more in the base (inner product: twice the row, so that
    the pair leads): equal exact values at the first ranks"""
    q[:n] = base[:n]
    base[5000:5000 + n] = base[6000:6000 + n] = base[:n] * np.float32(1.0 if metric == api.METRIC_L2 else 2.0)


def _kind(kind, n, seed):
    return _rows("sift", n, 128, seed) if kind == "sift" else _data("gauss20", n, 128, seed)


# ---- query counts: fewer than a workgroup's four, tails that are no multiple of 4 or 8, with and without qperm ------------------
@pytest.mark.parametrize("metric", [api.METRIC_L2, api.METRIC_IP])
def test_query_counts(metric):
    base = _rows("sift", N, 128, 610)
    q = _rows("sift", 67, 128, 611)
    _tied(base, q, metric)
    g = _handle("sift", base, metric)
    try:
        flagged = 0
        for nq in (1, 3, 4, 5, 61, 64, 67):
            flagged += _four(g, q[:nq], 10, 200, metric)[2]["replayed"]
        assert flagged > 0
        assert g.rerank_filter_form()["wave_calls"] == 7
        # the automatic rule on either side of its threshold (the forced forms say the same there as everywhere)
        amin = g.rerank_filter_form()["auto_min_nq"]
        assert 67 < amin <= 16384   # (the flagship call takes the wave form)
        big = np.tile(q, (amin // len(q) + 1, 1))[:amin]
        w0 = g.rerank_filter_form()["wave_calls"]
        _four(g, big[:amin - 1], 10, 200, metric)
        assert g.rerank_filter_form()["wave_calls"] == w0 + 1
        _four(g, big, 10, 200, metric)
        assert g.rerank_filter_form()["wave_calls"] == w0 + 3
    finally:
        g.close()


@pytest.mark.parametrize("metric", [api.METRIC_L2, api.METRIC_IP])
def test_query_counts_of_an_ordered_batch(metric):
    """the handle of test_gpu_rerank_filter_shapes.py whose batches are ordered from 256 queries on: the kernel runs them through
    qperm, an eighth of the order per XCD; 256 + n queries, n as above"""
    base, g = _ordered_case(metric)
    try:
        q = _data("gauss", 256 + 67, 128, 620)
        q[:8] = base[:8]
        flagged = 0
        for n in (1, 3, 4, 5, 61, 64, 67):
            flagged += _four(g, q[:256 + n], 10, 200, metric, nprobe=P_C)[2]["replayed"]
        assert flagged > 0
    finally:
        g.close()


# ---- short-list and k ----------------------------------------------------------------------------------------------------------
RS_W, KS_W = (1, 7, 8, 9, 63, 64, 65, 200, 255, 256, 257), (1, 10, 15, 16, 63)


@pytest.mark.parametrize("metric", [api.METRIC_L2, api.METRIC_IP])
@pytest.mark.parametrize("kind", ["sift", "gauss20"])
def test_short_lists_and_k(kind, metric):
    """the 8-lane groups' last partial round (R 1, 7, 8, 9), the head switch of tau at K1 16 / 17 and R 64 / 65, K1 = R, the last R
    the wave form admits and the first that falls back.  Sift-like integers: the image is exact and ties abound; Gaussian rows
    * 20 + 1000: err > 0, lo != 0."""
    base = _kind(kind, N, 630)
    q = _kind(kind, 7, 631)
    _tied(base, q, metric)
    g = _handle(kind, base, metric)
    try:
        # whatever the metric and the lists make of the rows above: the raw row of every query's second result becomes that
        # of its first (the lists index the clean vectors), equal exact values at the first two ranks
        args = api.SearchArgs(metric=metric, nprobe=P, recall_num=200, has_rank=True, exact_ties=1, **WIDE)
        _, I, _ = _search(g, 0, q, 2, args)
        assert (I >= 0).all()
        for a, b in I:
            g.raw_update(int(b), base[a])
        flagged = 0
        for R in RS_W:
            for k in KS_W:
                flagged += _four(g, q, k, R, metric)[2]["replayed"]
        assert flagged > 0
        f = g.rerank_filter_form()
        # per (R, k): form 2 runs the wave kernel iff max(R, k) <= 256 -- every pair here but R = 257
        assert f["wave_calls"] == (len(RS_W) - 1) * len(KS_W), f
    finally:
        g.close()


# ---- more than 64 survivors ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [api.METRIC_L2, api.METRIC_IP])
def test_more_than_64_survivors(metric):
    """300 rows equal to each query's row (inner product: twice the row, so that they lead), every list probed: with R = 200 every
    candidate ties and none can be proven out -- the path that sorts all the items of the wave instead of one run of 64"""
    base = _rows("sift", N, 128, 640)
    q = base[:4].copy()
    for i in range(4):
        base[1000 + 300 * i:1300 + 300 * i] = q[i] * np.float32(1.0 if metric == api.METRIC_L2 else 2.0)
    g = _handle("sift", base, metric)
    try:
        for k in (10, 63):
            D, I, t, surv = _four(g, q, k, 200, metric, nprobe=NLIST)
            assert surv >= 3 * 4 * 65, (k, surv)   # three filtered calls of four queries
            assert t["replayed"] > 0 and (I >= 0).all()
            assert (((I >= 1000) & (I < 2200)) | (I < 4)).all()   # (L2: rows 0 .. 3 are the queries themselves)
            if metric == api.METRIC_L2:
                assert (D == 0).all()
    finally:
        g.close()


# ---- ids of -1, a score window, rows that are not numbers ------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [api.METRIC_L2, api.METRIC_IP])
def test_fewer_candidates_a_window_and_non_finite_rows(metric):
    base = _rows("gauss", N, 128, 650)
    q = _rows("gauss", NQ, 128, 651)
    _tied(base, q, metric)
    g = _handle("gauss", base, metric)
    l2 = metric == api.METRIC_L2
    try:
        # one probed list of about 310 rows, some of fewer than 256: the table ends in ids of -1
        D, I, _, _ = _four(g, q, 10, 256, metric, nprobe=1)
        ids, n = _last_recall_ids(g, NQ, 256)
        assert n == NQ and (ids == -1).any() and (ids >= 0).any()
        # a window that cuts the short-list in half, both edges on a candidate's own value
        _four(g, q, 10, 200, metric)
        ids, n = _last_recall_ids(g, NQ, 200)
        val, _ = exact_values(q, base, ids, l2)
        v = np.sort(val[np.isfinite(val)])
        lo, hi = float(v[len(v) // 4]), float(v[3 * len(v) // 4])
        for k in (10, 63):   # (10 queries: with k 63 few candidates are certainly inside, most survive -- below the feedback's 4096)
            Dw, Iw, _, _ = _four(g, q[:10], k, 200, metric, min_score=lo, max_score=hi)
            assert ((Iw < 0) | ((Dw >= np.float32(lo)) & (Dw <= np.float32(hi)))).all() and (Iw >= 0).any()
        # a row of NaN and a row of +inf among the candidates (the lists index the clean vectors)
        bad_nan, bad_inf = int(I[20, 0]), int(I[21, 0])
        assert bad_nan >= 0 and bad_inf >= 0 and bad_nan != bad_inf
        g.raw_update(bad_nan, np.full(128, np.nan, np.float32))
        g.raw_update(bad_inf, np.full(128, np.inf, np.float32))
        for k in (1, 10):
            Db, Ib, _, _ = _four(g, q, k, 200, metric)
            assert np.isfinite(Db[Ib >= 0]).all() and not (Ib == bad_nan).any()
            if l2:
                assert not (Ib == bad_inf).any()
    finally:
        g.close()


# ---- the form switched under load ------------------------------------------------------------------------------------------------
def test_form_switch_under_load():
    """six callers of ivfpq_search_device_wait on one handle; caller 0 switches the form between its calls -- workgroup kernel,
    wave form, in turn -- while the other five search: every result is the plain call's.  Nobody else sets the form, so caller
    0's own calls run the kernel it asked for: both kernels run, whatever the interleaving."""
    import torch
    base = _rows("sift", N, 128, 660)
    base[N // 2:] = base[:N // 2]   # every vector twice: every call has a tie replay
    g = _handle("sift", base, api.METRIC_L2)
    try:
        dev = torch.device("cuda", 0)
        nthreads, nq, k, ncalls = 6, 67, 10, 8
        args = api.SearchArgs(metric=api.METRIC_L2, nprobe=P, recall_num=200, has_rank=True, exact_ties=1, **WIDE)
        qs = [torch.from_numpy(_rows("sift", nq, 128, 661 + t)).to(dev) for t in range(nthreads)]
        D0 = torch.empty((nq, k), dtype=torch.float32, device=dev)
        I0 = torch.empty((nq, k), dtype=torch.int64, device=dev)
        want = []
        g.set_rerank_filter(0)
        for t in range(nthreads):
            g.ivfpq_search_device(qs[t].data_ptr(), nq, k, args, D0.data_ptr(), I0.data_ptr())
            g.synchronize()
            want.append((D0.cpu().numpy().copy(), I0.cpu().numpy().copy()))
        g.set_rerank_filter(2)
        f0 = g.rerank_filter_form()["wave_calls"]
        errors = []

        def client(t):
            try:
                Dt = torch.empty((nq, k), dtype=torch.float32, device=dev)
                It = torch.empty((nq, k), dtype=torch.int64, device=dev)
                st = torch.cuda.Stream(device=dev)
                for rep in range(ncalls):
                    if t == 0:
                        g.set_rerank_filter_form(1 + rep % 2)
                    g.ivfpq_search_device_wait(qs[t].data_ptr(), nq, k, args, Dt.data_ptr(), It.data_ptr())
                    with torch.cuda.stream(st):
                        Dh, Ih = Dt.to("cpu", non_blocking=False), It.to("cpu", non_blocking=False)
                    if Dh.numpy().tobytes() != want[t][0].tobytes() or Ih.numpy().tobytes() != want[t][1].tobytes():
                        raise AssertionError("result bytes differ from the plain call's (thread %d, call %d)" % (t, rep))
            except BaseException as e:   # noqa: B902
                errors.append((t, repr(e)))

        th = [threading.Thread(target=client, args=(t,)) for t in range(nthreads)]
        c0 = g.rerank_filter_stats()["calls"]
        for x in th:
            x.start()
        for x in th:
            x.join()
        assert not errors, errors[:3]
        st, f = g.rerank_filter_stats(), g.rerank_filter_form()
        assert st["backoffs"] == 0 and st["calls"] - c0 == nthreads * ncalls
        assert ncalls // 2 <= f["wave_calls"] - f0 <= nthreads * ncalls - ncalls // 2, f
        print("form switch under load: %d filtered calls, %d of them in the wave form" % (st["calls"], f["wave_calls"] - f0))
    finally:
        g.close()
