"""GPU: the exact re-rank behind the byte image of a dense fp32 raw store (csrc/rerank_filter.hip, set_rerank_filter).

The filter only decides which candidates get the exact arithmetic, so the check is strict and needs no oracle: on ONE handle,
mode 2 (filter forced) answers byte for byte what mode 0 (the plain kernel) answers -- distances, labels, and the exact-tie
bookkeeping (tie_stats: cut ties, queries flagged and replayed).  Every search runs with exact ties on and the small path off,
which sends a batch of 64 queries through the fused re-rank kernel; rerank_filter_stats says whether the filter really ran.

Shapes: 20 000 rows, 64 lists, M = 16, 64 queries, recall_num in {11, 64, 200}, k in {1, 10, 63} (recall_num 11 with k 63 is the
R < k + 1 case: R = max(recall_num, k))."""
import threading

import numpy as np
import pytest

from gamma_amd import api, synth

pytestmark = pytest.mark.gpu

N, NLIST, M, NQ, P = 20000, 64, 16, 64, 8
RS, KS = (11, 64, 200), (1, 10, 63)
WIDE = dict(min_score=-3e38, max_score=3e38)
_trained = {}


def _rows(kind, n, d, seed):
    rng = np.random.default_rng(seed)
    if kind == "sift":
        return synth.sift_like(n, d=d, seed=seed)
    return rng.standard_normal((n, d)).astype(np.float32)


def _train(tag, base, d, nlist=NLIST, m=M):
    key = (tag, d, nlist, m)
    if key not in _trained:
        x = base[:4000] if len(base) >= 4000 else _rows(tag, 4000, d, 999)
        _trained[key] = api.train_ivfpq(x, nlist, m)
    return _trained[key]


def _handle(tag, base, metric, raw=None, dtype="float32", nlist=NLIST, m=M):
    d = base.shape[1]
    cc, pq = _train(tag, base, d, nlist, m)
    g = api.GammaHip(0)
    g.ivfpq_init(d, nlist, m, 8, metric)
    g.ivfpq_set_trained(cc, pq, None)
    g.raw_init(d, dtype)
    g.raw_append(base if raw is None else raw)
    g.add(base, 0)
    g.set_small_path(False)
    return g


def _search(g, mode, q, k, args):
    g.set_rerank_filter(mode)
    g.tie_stats(reset=True)
    D, I = g.ivfpq_search(q, k, args)
    return D, I, g.tie_stats(reset=True)


def _both(g, q, k, R, metric, filtered=True, nprobe=P, **win):
    """mode 0 against mode 2 on the same handle; returns mode 0's result"""
    args = api.SearchArgs(metric=metric, nprobe=nprobe, recall_num=R, has_rank=True, exact_ties=1, **(win or WIDE))
    D0, I0, t0 = _search(g, 0, q, k, args)
    c0 = g.rerank_filter_stats()
    D2, I2, t2 = _search(g, 2, q, k, args)
    c1 = g.rerank_filter_stats()
    assert D0.tobytes() == D2.tobytes() and I0.tobytes() == I2.tobytes(), (k, R)
    assert t0 == t2, (t0, t2)
    if filtered is not None:
        assert (c1["calls"] + c1["backoffs"] > c0["calls"] + c0["backoffs"]) == filtered
    return D0, I0, t0


@pytest.mark.parametrize("metric", [api.METRIC_L2, api.METRIC_IP])
@pytest.mark.parametrize("kind", ["sift", "gauss"])
@pytest.mark.parametrize("d", [128, 48, 272])
def test_filtered_rerank_is_the_plain_rerank(d, kind, metric):
    """d = 128: the register form, 48 and 272: the generic one.  Sift-like integers: the image is exact, ties abound and the
    flags must match; Gaussian floats: err > 0."""
    base = _rows(kind, N, d, 10 + d)
    q = _rows(kind, NQ, d, 77 + d)
    q[:8] = base[:8]   # queries that are rows, and each of those rows twice: ties at the first two ranks
    base[5000:5008] = base[:8]
    g = _handle(kind, base, metric)
    try:
        flagged = 0
        for R in RS:
            for k in KS:
                flagged += _both(g, q, k, R, metric)[2]["replayed"]
        st = g.rerank_filter_stats()
        assert st["image_rows"] == N and st["candidates"] > 0 and st["calls"] >= 1
        print("d %d %s metric %d: %d of %d candidates survived, %d calls, %d back-offs, %d queries flagged" % (
            d, kind, metric, st["survivors"], st["candidates"], st["calls"], st["backoffs"], flagged))
        assert flagged > 0
    finally:
        g.close()


def test_rows_outside_the_image_range_are_found():
    """Rows appended after the image exists, far outside its range: they clamp, their error is honest, they are found."""
    d = 128
    base = _rows("gauss", N, d, 3)
    g = _handle("gauss", base, api.METRIC_L2)
    try:
        q = _rows("gauss", NQ, d, 4)
        _both(g, q, 10, 200, api.METRIC_L2)
        assert g.rerank_filter_stats()["image_rows"] == N
        far = (_rows("gauss", 128, d, 5) * 3 + np.float32(500.0)).astype(np.float32)   # (fewer than recall_num: all candidates)
        g.raw_append(far)
        g.add(far, N)
        assert g.rerank_filter_stats()["image_rows"] == N + 128
        qf = (far[:NQ] + _rows("gauss", NQ, d, 6) * np.float32(0.01)).astype(np.float32)
        for k in (1, 10):
            D, I, _ = _both(g, qf, k, 200, api.METRIC_L2, nprobe=NLIST)
            assert np.array_equal(I[:, 0], N + np.arange(NQ))
        _both(g, q, 10, 200, api.METRIC_L2)
    finally:
        g.close()


@pytest.mark.parametrize("metric", [api.METRIC_L2, api.METRIC_IP])
def test_duplicated_rows_across_the_k_boundary(metric):
    """groups of 12 equal rows: k = 10 and k = 11 cut through a group, the k + 1 test looks at its other half"""
    d = 128
    base = _rows("sift", N, d, 8)
    for i in range(40):
        base[100 * i:100 * i + 12] = base[100 * i]
    g = _handle("sift", base, metric)
    try:
        q = base[0:4000:100][:NQ // 2]
        q = np.concatenate([q, q + np.float32(1.0)])
        tot = 0
        for k in (10, 11, 12, 13):
            tot += _both(g, q, k, 200, metric, nprobe=NLIST)[2]["replayed"]
        assert tot > 0
    finally:
        g.close()


@pytest.mark.parametrize("kind", ["sift", "gauss"])
@pytest.mark.parametrize("metric", [api.METRIC_L2, api.METRIC_IP])
def test_score_window_cuts_through_the_candidates(metric, kind):
    """both edges of the window lie among the exact values of the candidates, some of them exactly on a candidate's value:
    which side a candidate is on is the exact value's decision"""
    d = 128
    base = _rows(kind, N, d, 12)
    q = _rows(kind, NQ, d, 13)
    g = _handle(kind, base, metric)
    try:
        D, I, _ = _both(g, q, 63, 200, metric)
        v = np.sort(D[I >= 0])
        for lo, hi in ((v[len(v) // 4], v[3 * len(v) // 4]), (float(np.median(D[:, 5])), float(np.median(D[:, 40]))),
                       (-3e38, v[len(v) // 2]), (v[len(v) // 2], 3e38)):
            lo, hi = min(lo, hi), max(lo, hi)
            for k in (1, 10):
                Dw, Iw, _ = _both(g, q, k, 200, metric, min_score=float(lo), max_score=float(hi))
                assert ((Iw < 0) | ((Dw >= lo) & (Dw <= hi))).all()
                assert (Iw >= 0).any()
    finally:
        g.close()


def test_unusable_candidates():
    """candidate ids of -1 (short lists: fewer candidates than recall_num, fewer than k + 1 for some queries) and ids at and
    beyond the row count (vectors indexed without a raw row)"""
    d, n = 128, 1500
    base = _rows("gauss", n, d, 21)
    g = _handle("gauss", base, api.METRIC_L2, raw=base[:n - 400])
    try:
        q = _rows("gauss", NQ, d, 22)
        short = 0
        for R in RS:
            for k in KS:
                D, I, _ = _both(g, q, k, R, api.METRIC_L2, nprobe=1)
                short += int((I < 0).any())
                assert (I < n - 400).all()
        assert short > 0
    finally:
        g.close()


def test_values_on_half_steps_and_neighbours_an_ulp_apart():
    """every value sits on a half step of the image (lo = 0, Delta = 1: the rounding goes either way) and the candidates
    come in pairs whose exact distances differ by an ulp or not at all"""
    d = 128
    rng = np.random.default_rng(31)
    half = (rng.integers(0, 255, size=(N // 2, d)) + 0.5).astype(np.float32)
    half[0, :] = 0.0
    half[1, :] = 255.0
    twin = half.copy()
    j = rng.integers(0, d, size=N // 2)
    twin[np.arange(N // 2), j] = np.nextafter(twin[np.arange(N // 2), j], np.float32(1e9))
    base = np.empty((N, d), np.float32)
    base[0::2], base[1::2] = half, twin
    g = _handle("half", base, api.METRIC_L2)
    try:
        q = (base[2:2 + 2 * NQ:2] + rng.integers(-3, 4, size=(NQ, d))).astype(np.float32)
        for k in (1, 2, 10, 63):
            _both(g, q, k, 200, api.METRIC_L2, nprobe=NLIST)
        st = g.rerank_filter_stats()
        assert st["calls"] >= 1 and st["survivors"] < st["candidates"]
    finally:
        g.close()


def test_writers_keep_the_image_in_step():
    d = 128
    base = _rows("gauss", N, d, 41)
    q = _rows("gauss", NQ, d, 42)
    g = _handle("gauss", base, api.METRIC_L2)
    try:
        _both(g, q, 10, 200, api.METRIC_L2)
        assert g.rerank_filter_stats()["image_rows"] == N
        more = _rows("gauss", 3000, d, 44)
        g.raw_append(more)                                         # raw_append (grows the image)
        g.add(more, N)
        _both(g, q, 10, 200, api.METRIC_L2)
        _, I, _ = _both(g, q, 10, 64, api.METRIC_L2)
        hit = np.unique(I[I >= 0])[:50]
        for v in hit[:5]:                                          # raw_update: rows the queries find move away
            g.raw_update(int(v), (base[0] * 0 + np.float32(40.0)).astype(np.float32))
        _both(g, q, 10, 200, api.METRIC_L2)
        owner = {int(I[i, c]): i for i, c in zip(*np.nonzero(I >= 0))}   # a query that has the row among its candidates
        g.raw_update_batch(hit, np.stack([q[owner[int(v)]] for v in hit]) + np.float32(0.001))   # ... and next to the queries
        D, _, _ = _both(g, q, 10, 200, api.METRIC_L2)
        assert (D[:, 0] < 1.0).sum() > 0
        g.raw_write(100, _rows("gauss", 500, d, 45) * np.float32(7.0))   # raw_write over rows, values beyond the range
        _both(g, q, 10, 200, api.METRIC_L2)
        assert g.rerank_filter_stats()["image_rows"] == N + 3000
        before = g.total_mem_bytes()
        g.raw_clear()                                              # raw_clear releases it; the next call builds a new one
        assert g.rerank_filter_stats()["image_rows"] == 0 and g.total_mem_bytes() < before
        g.raw_append(np.concatenate([base, more]))
        _both(g, q, 10, 200, api.METRIC_L2)
        assert g.rerank_filter_stats()["image_rows"] == N + 3000
    finally:
        g.close()


def test_image_memory_is_counted_once_it_exists():
    d = 128
    base = _rows("gauss", N, d, 51)
    g = _handle("gauss", base, api.METRIC_L2)
    try:
        m0 = g.total_mem_bytes()
        args = api.SearchArgs(metric=api.METRIC_L2, nprobe=P, recall_num=200, exact_ties=1, **WIDE)
        g.ivfpq_search(base[:NQ], 10, args)        # mode 1: a small call builds nothing
        assert g.total_mem_bytes() == m0 and g.rerank_filter_stats()["image_rows"] == 0
        g.set_rerank_filter(2)
        g.ivfpq_search(base[:NQ], 10, args)
        cap = g.raw_stats()["capacity"]
        assert g.total_mem_bytes() == m0 + cap * (d + 8)
    finally:
        g.close()


def test_search_beside_an_appending_writer():
    d = 128
    base = _rows("gauss", N, d, 61)
    q = base[:NQ] + np.float32(0.001)
    g = _handle("gauss", base, api.METRIC_L2)
    try:
        g.set_rerank_filter(2)
        args = api.SearchArgs(metric=api.METRIC_L2, nprobe=P, recall_num=200, exact_ties=1, **WIDE)
        g.ivfpq_search(q, 10, args)
        stop, bad, calls = threading.Event(), [], [0]

        def searcher():
            while not stop.is_set():
                D, I = g.ivfpq_search(q, 10, args)
                calls[0] += 1
                if not np.array_equal(I[:, 0], np.arange(NQ)):   # the appended rows are far away
                    bad.append(I[:, 0].copy())

        t = threading.Thread(target=searcher)
        t.start()
        try:
            for b in range(12):
                blk = _rows("gauss", 4000, d, 70 + b) + np.float32(100.0)
                g.raw_append(blk)
                g.add(blk, N + 4000 * b)
        finally:
            stop.set()
            t.join()
        assert not bad and calls[0] > 0
        assert g.rerank_filter_stats()["image_rows"] == N + 48000
        _both(g, q, 10, 200, api.METRIC_L2)
    finally:
        g.close()


def test_stores_without_an_image():
    """float16 rows, rows of 100 floats and a sparse store: no image, unchanged answers"""
    for d, dtype, m in ((128, "float16", 16), (100, "float32", 4)):
        base = _rows("sift", 6000, d, 81)
        g = _handle("sift", base, api.METRIC_L2, dtype=dtype, nlist=16, m=m)
        try:
            _both(g, base[:NQ] + np.float32(1.0), 10, 200, api.METRIC_L2, filtered=False)
            st = g.rerank_filter_stats()
            assert st["image_rows"] == 0 and st["calls"] == 0 and st["candidates"] == 0
        finally:
            g.close()
    d = 128
    base = _rows("sift", 6000, d, 82)
    cc, pq = _train("sift", base, d, 16, 16)
    g = api.GammaHip(0)
    try:
        g.ivfpq_init(d, 16, 16, 8, api.METRIC_L2)
        g.ivfpq_set_trained(cc, pq, None)
        g.raw_init(d)
        g.raw_put(np.arange(0, 6000, 2), base[0::2])
        g.add(base, 0)
        g.set_small_path(False)
        g.set_rerank_filter(2)
        with pytest.raises(api.GammaHipError):
            g.ivfpq_search(base[:NQ], 10, api.SearchArgs(metric=api.METRIC_L2, nprobe=4, recall_num=200, exact_ties=1, **WIDE))
        assert g.rerank_filter_stats()["image_rows"] == 0
    finally:
        g.close()


def test_the_handle_backs_off_when_everything_survives():
    """the image's range is fixed on small values, then every row is rewritten 10 000 times larger: all of them clamp, no
    candidate is proven out, and the handle returns to the plain kernel -- same answers"""
    d = 128
    small = _rows("gauss", N, d, 91)
    g = _handle("gauss", small, api.METRIC_L2)
    try:
        q = _rows("gauss", NQ, d, 92)
        _both(g, q, 10, 200, api.METRIC_L2)
        s0 = g.rerank_filter_stats()
        assert s0["calls"] == 1 and s0["backoffs"] == 0 and 2 * s0["survivors"] < s0["candidates"]
        g.raw_write(0, small * np.float32(1e4))
        args = api.SearchArgs(metric=api.METRIC_L2, nprobe=P, recall_num=200, exact_ties=1, **WIDE)
        D0, I0, _ = _search(g, 0, q, 10, args)
        g.set_rerank_filter(2)   # (once: the setter makes the next call probe)
        for _ in range(4):
            D, I = g.ivfpq_search(q, 10, args)
            assert D.tobytes() == D0.tobytes() and I.tobytes() == I0.tobytes()
        s1 = g.rerank_filter_stats()
        # the first call ran the filter and every candidate survived it; the second read that and backed off
        assert s1["backoffs"] == 1 and s1["calls"] == 2
        assert s1["survivors"] - s0["survivors"] == s1["candidates"] - s0["candidates"] == NQ * 200
    finally:
        g.close()
