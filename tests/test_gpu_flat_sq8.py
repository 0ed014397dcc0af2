"""GPU: flat search over a scalar-quantised raw store (gamma_hip_set_flat_sq8_rows).

The store is lossy and nothing else is: it holds W = sq8_ref.decode(sq8_ref.encode(base)), a code is decoded as it is loaded (a
multiply, then an add, each rounded in fp32) and every distance is fvec_L2sqr / fvec_inner_product of the fp32 query and the
decoded row.  So the results must be
  * the CPU oracle's flat search over W, labels and distance bits at every rank (compare_exact, exact ties on), and
  * byte-identical to those of a second handle whose fp32 store holds W.
The ranges are the minimum / maximum of HALF of the rows, so the other half clips at both ends, and one dimension is constant
(vmin == vmax, step 0).  Shapes are the smallest at which each reader of rows on the flat path can go wrong (see the docstrings;
they are those of tests/test_gpu_flat_rows.py and tests/test_gpu_flat_anyd.py)."""
import numpy as np
import pytest

from gamma_amd import _lib, api
from oracle import binding as B
from tests import sq8_ref as S
from tests.parity import compare_exact

pytestmark = pytest.mark.gpu

WIDE = dict(min_score=-3e38, max_score=3e38)
EUNSUPPORTED = -6   # include/gamma_hip.h
METRICS = (B.METRIC_L2, B.METRIC_IP)


def ranged(x, half=None):
    """(x, vmin, vmax): the ranges are the minimum / maximum of the first half of the rows (or of `half`)"""
    h = x[:len(x) // 2] if half is None else half
    return np.ascontiguousarray(x, np.float32), h.min(axis=0), h.max(axis=0)


def random_rows(n, d, seed):
    """sq8_ref.rows: a scale and an offset per dimension, one dimension constant; the second half is drawn wider and clips"""
    x = np.concatenate([S.rows(n // 2, d, seed), S.rows(n - n // 2, d, seed + 1, wide=1.6)])
    x, vmin, vmax = ranged(x)
    step, inv = S.params(vmin, vmax)
    codes = S.encode(x[n // 2:], vmin, inv)
    assert (codes == 0).any() and (codes == 255).any() and (step == 0).sum() == 1
    return x, vmin, vmax


def random_queries(n, d, seed):
    return S.rows(n, d, seed)


def margin_rows(n, d, kind, seed, nq, nproto=200, noise=0.05):
    """data that sits on the matrix filter's margin.  near_duplicates: prototypes on the code grid plus noise of `noise` steps --
    below half a step, every row of a prototype decodes to the same W row (many exact ties; the first half of the rows comes
    from half of the prototypes, so the others clip); above, the rows differ in a few codes.  unit: unit-norm embeddings."""
    rng = np.random.default_rng(seed)
    if kind == "unit":
        base = rng.standard_normal((n, d)).astype(np.float32)
        base /= np.linalg.norm(base, axis=1, keepdims=True)
        base[:, min(5, d - 1)] = np.float32(0.03125)      # the constant dimension
        q = rng.standard_normal((nq, d)).astype(np.float32)
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        return ranged(base) + (q,)
    P = S.rows(nproto, d, seed)
    lo, hi = P[:nproto // 2].min(axis=0), P[:nproto // 2].max(axis=0)
    step, inv = S.params(lo, hi)
    P = S.decode(S.encode(P, lo, inv), lo, step)           # on the grid of the first half's ranges
    idx = np.concatenate([rng.integers(0, nproto // 2, n // 2), rng.integers(0, nproto, n - n // 2)])
    base = (P[idx] + rng.uniform(-noise, noise, (n, d)).astype(np.float32) * step).astype(np.float32)
    # the other half of the prototypes reaches beyond the ranges where it sits at their ends: those values clip to the same code
    codes, far = S.encode(P, lo, inv)[idx], (idx >= nproto // 2)[:, None]
    base = (base + np.where(far & (codes == 255), 5, 0) * step - np.where(far & (codes == 0), 5, 0) * step).astype(np.float32)
    assert (base[n // 2:] > base[:n // 2].max(axis=0)).any() and (base[n // 2:] < base[:n // 2].min(axis=0)).any()
    q = (P[rng.integers(0, nproto, nq)] + rng.standard_normal((nq, d)).astype(np.float32) * np.float32(3.0) * step).astype(np.float32)
    return ranged(base) + (q,)


class Pair:
    """the sq8 store under test, appended the fp32 rows x, and the fp32 store of the rows it holds, W"""

    def __init__(self, x, vmin, vmax, small_path=None, dist_budget=None):
        self.x, self.vmin, self.vmax = x, vmin, vmax
        self.W = np.ascontiguousarray(S.stored(x, vmin, vmax))
        assert np.isfinite(self.W).all()
        self.g = api.GammaHip(0)
        self.g32 = api.GammaHip(0)
        d = x.shape[1]
        self.g.raw_init(d, "sq8")
        self.g.raw_sq8_set_ranges(vmin, vmax)
        self.g.set_flat_sq8_rows(True)
        self.g.raw_append(x)
        self.g32.raw_init(d)
        self.g32.raw_append(self.W)
        for h in (self.g, self.g32):
            if small_path is not None:
                h.set_small_path(small_path)
            if dist_budget is not None:
                h.set_dist_budget(dist_budget)
        assert self.g.raw_elem_type() == 4 and self.g32.raw_elem_type() == 0

    def close(self):
        self.g.close()
        self.g32.close()

    def check(self, q, k, metric, win=WIDE, bm=None, docs=None):
        ctx_kw, kw = {}, {}
        if bm is not None:
            ctx_kw["docids_bitmap"] = bm
        if docs is not None:
            ctx_kw["range_filters"] = [B.make_range_filter(docs)]
            kw["range_filters"] = [api.make_range_filter(docs)]
        D, I = B.flat_search(self.W, q, k, metric, B.make_ctx(**win, **ctx_kw))
        args = api.SearchArgs(metric=metric, **win, **kw)
        Dg, Ig = self.g.flat_search(q, k, args)
        D32, I32 = self.g32.flat_search(q, k, args)
        compare_exact(D, I, Dg, Ig)
        assert Dg.tobytes() == D32.tobytes() and Ig.tobytes() == I32.tobytes()
        return D, I


def bitmap_of(n, dead):
    bm = np.zeros((n >> 3) + 1, dtype=np.uint8)
    np.bitwise_or.at(bm, dead >> 3, (1 << (dead & 7)).astype(np.uint8))
    return bm


# ---- 1. the switch ----------------------------------------------------------------------------------------------------
def test_switch_turns_flat_search_over_sq8_rows_on():
    """off (the default): EUNSUPPORTED with the sq8 store's refusal message, as before, and gamma_hip_set_flat_narrow_rows alone
    changes nothing; on: served; off again: refused again.  With the switch on, raw_put and the IVFFLAT search still refuse."""
    d, N = 24, 700
    x, vmin, vmax = random_rows(N, d, 1)
    W = S.stored(x, vmin, vmax)
    q = random_queries(8, d, 2)
    g = api.GammaHip(0)
    L = g.L
    args = api.SearchArgs(metric=api.METRIC_L2, **WIDE)
    D = np.empty((8, 5), np.float32)
    I = np.empty((8, 5), np.int64)

    def flat():
        return L.gamma_hip_flat_search(g.h, args.ref(), 8, q.ctypes.data_as(_lib.f32p), 5, D.ctypes.data_as(_lib.f32p),
                                       I.ctypes.data_as(_lib.i64p))

    def refused(rc, what=b"reads fp32 rows"):
        msg = L.gamma_hip_last_error(g.h)
        assert rc == EUNSUPPORTED and b"sq8" in msg and b"gamma_hip_raw_init_sq8" in msg and what in msg, (rc, msg)

    try:
        g.raw_init(d, "sq8")
        g.raw_sq8_set_ranges(vmin, vmax)
        g.raw_append(x)
        refused(flat())
        g.set_flat_narrow_rows(True)      # the other narrow stores' switch: not this store's
        refused(flat())
        g.set_flat_narrow_rows(False)
        g.set_flat_sq8_rows(True)
        assert flat() == 0
        Do, Io = B.flat_search(W, q, 5, B.METRIC_L2, B.make_ctx(**WIDE))
        compare_exact(Do, Io, D, I)
        vids = np.arange(4, dtype=np.int64)
        refused(L.gamma_hip_raw_put(g.h, 4, vids.ctypes.data_as(_lib.i64p), x[:4].ctypes.data_as(_lib.f32p)), b"")
        refused(L.gamma_hip_raw_drop(g.h, 4, vids.ctypes.data_as(_lib.i64p)), b"")
        g.set_flat_sq8_rows(False)
        refused(flat())
    finally:
        g.close()
    g = api.GammaHip(0)
    L = g.L
    try:
        g.ivfflat_init(d, 4, api.METRIC_L2)
        g.ivfflat_set_trained(np.ascontiguousarray(W[:4]))
        g.raw_init(d, "sq8")
        g.raw_sq8_set_ranges(vmin, vmax)
        g.set_flat_sq8_rows(True)
        g.set_ivfflat_narrow_rows(True)
        g.raw_append(x[:500])
        g.add_keys_batch([0], [500], np.arange(500), np.zeros((500, 1), np.uint8))
        refused(L.gamma_hip_ivfflat_search(g.h, args.ref(), 8, q.ctypes.data_as(_lib.f32p), 5, D.ctypes.data_as(_lib.f32p),
                                           I.ctypes.data_as(_lib.i64p)))
    finally:
        g.close()


@pytest.mark.parametrize("dtype", ["float32", "uint8"])
def test_switch_leaves_the_other_stores_alone(dtype):
    """an fp32 store, and a uint8 store behind gamma_hip_set_flat_narrow_rows, answer byte for byte the same with the new switch
    on and off; the uint8 store without ITS switch stays refused whatever the new one says"""
    d, N = 32, 900
    W = np.random.default_rng(3).integers(0, 256, size=(N, d)).astype(np.float32)
    q = (127.0 + 60.0 * np.random.default_rng(4).standard_normal((8, d))).astype(np.float32)
    args = api.SearchArgs(metric=api.METRIC_L2, **WIDE)
    g = api.GammaHip(0)
    try:
        g.raw_init(d, dtype)
        g.raw_append(W)
        if dtype == "uint8":
            g.set_flat_sq8_rows(True)
            with pytest.raises(Exception):
                g.flat_search(q, 5, args)
            g.set_flat_sq8_rows(False)
            g.set_flat_narrow_rows(True)
        r0 = g.flat_search(q, 5, args)
        g.set_flat_sq8_rows(True)
        r1 = g.flat_search(q, 5, args)
        g.set_flat_sq8_rows(False)
        r2 = g.flat_search(q, 5, args)
        assert r0[0].tobytes() == r1[0].tobytes() == r2[0].tobytes() and r0[1].tobytes() == r1[1].tobytes() == r2[1].tobytes()
        Do, Io = B.flat_search(W, q, 5, B.METRIC_L2, B.make_ctx(**WIDE))
        compare_exact(Do, Io, *r1)
    finally:
        g.close()


# ---- 2. the slab kernels (kernels.hip) --------------------------------------------------------------------------------
# N = 3001: a partial block of 128 (k_pairwise_lds) and of 256 rows (k_pairwise_rowreg / _generic).  nq = 16 goes to
# k_pairwise_lds for d in {128, 96, 16} (two threads per row, 16-byte loads) and to k_pairwise_generic otherwise: d = 20 (rows
# aligned to 4 bytes), d = 33 (rows aligned to a byte).  nq = 5: fewer than 8 queries per workgroup, so the same d goes to
# k_pairwise_rowreg.
@pytest.mark.parametrize("d,nq", [(128, 16), (96, 16), (16, 16), (20, 16), (33, 16), (64, 5), (16, 5)])
def test_slab_kernels_over_sq8_rows(d, nq):
    N = 3001
    x, vmin, vmax = random_rows(N, d, 10 + d)
    q = random_queries(nq, d, 11 + d)
    rng = np.random.default_rng(d)
    bm = bitmap_of(N, rng.choice(N, N // 9, replace=False))
    docs = rng.choice(N, 3 * N // 4, replace=False)
    for small_path in (1, 0):   # one row chunk + the small tail | the chunked path (one chunk, no bound at this N)
        p = Pair(x, vmin, vmax, small_path=small_path)
        try:
            for metric in METRICS:
                for k in (1, 100):
                    p.check(q, k, metric)
            p.g.bitmap_upload(bm, N)
            p.g32.bitmap_upload(bm, N)
            for metric in METRICS:
                Dw, _ = p.check(q, 100, metric, bm=bm, docs=docs)
                win = dict(min_score=float(np.quantile(Dw, 0.2)), max_score=float(np.quantile(Dw, 0.9)))
                p.check(q, 100, metric, win=win, bm=bm, docs=docs)
        finally:
            p.close()


# ---- 3. the emitting kernel -------------------------------------------------------------------------------------------
def test_emitting_kernel_over_sq8_rows():
    """d = 16 with 24 queries has no matrix variant: the first chunk is 65536 rows, the remaining 4464 go through
    k_pairwise_lds<.., EMIT> under the running bound (the small path is switched off)"""
    d, N, nq = 16, 70000, 24
    x, vmin, vmax = random_rows(N, d, 21)
    q = random_queries(nq, d, 22)
    p = Pair(x, vmin, vmax, small_path=0)
    try:
        for metric in METRICS:
            p.check(q, 10, metric)
    finally:
        p.close()


# ---- 4. the matrix-pipe filter (flat_mfma.hip) ------------------------------------------------------------------------
# nq = 96: more than the small path's 64 queries, and a padded tile of 64.  N = 21000: the first chunk is 16384 rows, then ONE
# pass of 4616 rows with a partial block of 128.
@pytest.mark.parametrize("kind", ["near_duplicates", "unit"])
@pytest.mark.parametrize("d", [32, 128])
def test_matrix_filter_over_sq8_rows_never_drops_a_neighbour(kind, d):
    N, nq = 21000, 96
    x, vmin, vmax, q = margin_rows(N, d, kind, 100 + d, nq)
    rng = np.random.default_rng(d)
    bm = bitmap_of(N, rng.choice(N, N // 11, replace=False))
    docs = rng.choice(N, 3 * N // 4, replace=False)
    p = Pair(x, vmin, vmax)
    try:
        if kind == "near_duplicates":      # many rows decode identically
            assert len(np.unique(p.W, axis=0)) <= 200
        for metric in METRICS:
            for k in (1, 10):
                p.check(q, k, metric)
        p.g.bitmap_upload(bm, N)
        p.g32.bitmap_upload(bm, N)
        for metric in METRICS:
            Dw, _ = p.check(q, 10, metric, bm=bm, docs=docs)
            p.check(q, 10, metric, win=dict(min_score=float(np.quantile(Dw, 0.2)), max_score=float(np.quantile(Dw, 0.9))),
                    bm=bm, docs=docs)
    finally:
        p.close()


@pytest.mark.parametrize("kind", ["near_duplicates", "unit"])
@pytest.mark.parametrize("d", [160, 1056])
def test_long_row_filter_over_sq8_rows(kind, d):
    """k_flat_filter_big: d = 160 (the image in LDS) and d = 1056 (the LO_L2 form); a first chunk of 1024 rows, then passes of
    3072 and 904 rows"""
    N, nq = 5000, 96
    x, vmin, vmax, q = margin_rows(N, d, kind, 200 + d, nq)
    p = Pair(x, vmin, vmax)
    try:
        for metric in METRICS:
            p.check(q, 10, metric)
    finally:
        p.close()


@pytest.mark.parametrize("kind", ["near_duplicates", "unit"])
@pytest.mark.parametrize("d", [100, 301, 2048])
def test_any_length_filter_over_sq8_rows(kind, d):
    """k_flat_filter_any: d = 100 (rows aligned to 4 bytes: element loads, d_pad = 128, the upper lanes' half row ends inside
    the padding), d = 301 (rows aligned to a byte, an odd number of table entries), d = 2048 (8-byte loads, part of the image read
    from the L2).  N = 6001: a partial step of 256 rows."""
    N, nq = 6001, 96
    x, vmin, vmax, q = margin_rows(N, d, kind, 300 + d, nq)
    p = Pair(x, vmin, vmax)
    try:
        for metric in METRICS:
            p.check(q, 10, metric)
    finally:
        p.close()


# ---- 5. ties at the cut -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS, ids=["l2", "ip"])
def test_overflow_redo_reads_sq8_rows(metric):
    """Rows in improving order for query 0: every row of the pass behind the first chunk beats the bound, the query's list
    (2048 items) overflows and the call is redone without a bound -- two row chunks through one slab, so the tie phase
    recomputes the flagged queries' rows (the redo branch of tie_phase).  Every distinct row occurs about 14 times, so every
    query has exact ties among its best.  That the list must overflow is shown on the CPU (the rows of the pass within the
    bound, against a capacity of 2048); that the redo ran is implied by that argument and not observed."""
    N, d, nq, k = 21000, 32, 96, 10
    pool, vmin, vmax, q = margin_rows(1500, d, "near_duplicates", 300, nq, nproto=50, noise=2.0)
    x = pool[np.random.default_rng(7).integers(0, len(pool), N)]      # every pool row about 14 times
    W = S.stored(x, vmin, vmax)
    assert len(np.unique(W, axis=0)) <= 1500 < N // 10                 # far fewer distinct rows than rows

    def score(W):      # smaller is better
        if metric == B.METRIC_L2:
            return ((W.astype(np.float64) - q[0].astype(np.float64)) ** 2).sum(1)
        return -(W.astype(np.float64) @ q[0].astype(np.float64))

    order = np.argsort(-score(W), kind="stable")
    x, W = np.ascontiguousarray(x[order]), np.ascontiguousarray(W[order])
    s0 = score(W)
    bound = np.sort(s0[:16384])[k]      # (k + 1 results are kept with exact ties on)
    assert int((s0[16384:] <= bound).sum()) > 2048
    p = Pair(x, vmin, vmax)
    try:
        assert np.array_equal(p.W, W)
        D, I = p.check(q, k, metric)
        assert (D[:, 0] == D[:, 1]).all()      # ties among the results: the tie phase had every query to replay
    finally:
        p.close()


def test_tie_recompute_over_several_chunks_reads_sq8_rows():
    """d = 20 with 24 queries has neither an emitting kernel nor a matrix variant, so 70000 rows go through one slab as two row
    chunks without a bound, and every query with a tie has its rows computed again by the tie phase (launch_pairwise_filtered
    over the whole store, k_pairwise_generic).  Every distinct row occurs about 35 times: every query is such a query."""
    N, d, nq, k = 70000, 20, 24, 10
    pool, vmin, vmax = random_rows(2000, d, 41)
    x = np.ascontiguousarray(pool[np.random.default_rng(8).integers(0, len(pool), N)])
    q = random_queries(nq, d, 42)
    p = Pair(x, vmin, vmax, small_path=0)
    try:
        assert len(np.unique(p.W, axis=0)) <= 2000 < N // 10
        for metric in METRICS:
            D, I = p.check(q, k, metric)
            assert (D[:, 0] == D[:, 1]).all()
    finally:
        p.close()


# ---- 6. writers and entry points --------------------------------------------------------------------------------------
def test_writers_and_device_entry_points():
    """after raw_update_batch the search sees the re-encoded rows; gamma_hip_flat_search_device and _device_wait give the host
    entry's bytes (N = 21000, d = 64, 96 queries: the matrix filter and its exact stage read the updated store)"""
    import torch
    N, d, nq, k = 21000, 64, 96, 10
    x, vmin, vmax = random_rows(N, d, 51)
    q = random_queries(nq, d, 52)
    p = Pair(x, vmin, vmax)
    try:
        p.check(q, k, B.METRIC_L2)
        vids = np.random.default_rng(9).choice(N, 300, replace=False).astype(np.int64)
        new = np.ascontiguousarray(q[np.arange(300) % nq] + S.rows(300, d, 53) * np.float32(0.01))   # near the queries: they enter the results
        p.g.raw_update_batch(vids, new)
        x2 = x.copy()
        x2[vids] = new
        p.W = np.ascontiguousarray(S.stored(x2, vmin, vmax))
        p.g32.raw_update_batch(vids, np.ascontiguousarray(p.W[vids]))
        for metric in METRICS:
            _, Io = p.check(q, k, metric)
            assert metric != B.METRIC_L2 or np.isin(Io, vids).any()
            args = api.SearchArgs(metric=metric, **WIDE)
            D, I = p.g.flat_search(q, k, args)
            tq = torch.from_numpy(q).cuda()
            for entry in (p.g.flat_search_device, p.g.flat_search_device_wait):
                tD = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
                tI = torch.zeros((nq, k), dtype=torch.int64, device="cuda")
                entry(tq.data_ptr(), nq, k, args, tD.data_ptr(), tI.data_ptr())
                torch.cuda.synchronize()
                assert tD.cpu().numpy().tobytes() == D.tobytes() and tI.cpu().numpy().tobytes() == I.tobytes()
    finally:
        p.close()
