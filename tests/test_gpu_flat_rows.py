"""GPU: flat search over a float16 / uint8 / int8 raw store (gamma_hip_set_flat_narrow_rows).

A narrow row widens to fp32 exactly and every distance is fvec_L2sqr / fvec_inner_product of the fp32 query and the widened row,
so with W = base.astype(T).astype(float32) the results must be
  * the CPU oracle's flat search over W, labels and distance bits at every rank (compare_exact, exact ties on), and
  * byte-identical to those of a second handle whose fp32 store holds W.
Shapes are the smallest at which each reader of rows on the flat path can go wrong (see the tests' docstrings)."""
import numpy as np
import pytest

from gamma_amd import _lib, api
from oracle import binding as B
from tests.parity import compare_exact

pytestmark = pytest.mark.gpu

WIDE = dict(min_score=-3e38, max_score=3e38)
DTYPES = ["float16", "uint8", "int8"]
NP = {"float16": np.float16, "uint8": np.uint8, "int8": np.int8}
RANGE = {"uint8": (0, 255), "int8": (-128, 127)}
EUNSUPPORTED = -6   # include/gamma_hip.h
METRICS = (B.METRIC_L2, B.METRIC_IP)


def widened(x, dtype):
    """W: what the store of this type holds for x, as fp32 (x must be inside the type's range)"""
    return np.ascontiguousarray(x.astype(NP[dtype]).astype(np.float32))


def random_rows(n, d, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == "float16":
        x = (rng.standard_normal((n, d)) * 3).astype(np.float32)
    else:
        lo, hi = RANGE[dtype]
        x = rng.integers(lo, hi + 1, size=(n, d)).astype(np.float32)
        x[0, 0], x[0, -1] = lo, hi
    return widened(x, dtype)


def random_queries(n, d, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == "float16":
        return (rng.standard_normal((n, d)) * 3).astype(np.float32)
    lo, hi = RANGE[dtype]
    return ((lo + hi) / 2.0 + 60.0 * rng.standard_normal((n, d))).astype(np.float32)


def margin_rows(n, d, dtype, kind, seed, nq):
    """data that sits on the matrix filter's margin: rows that are tiny perturbations of a few prototypes -- for bytes the
    noise is {-1, 0, 1}, for float16 the perturbed rows are rounded to half (many exact ties either way); `unit`: unit-norm
    embeddings rounded to half"""
    rng = np.random.default_rng(seed)
    if kind == "unit":
        base = rng.standard_normal((n, d)).astype(np.float32)
        base /= np.linalg.norm(base, axis=1, keepdims=True)
        q = rng.standard_normal((nq, d)).astype(np.float32)
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        return widened(base, dtype), q
    if dtype == "float16":
        proto = (rng.standard_normal((50, d)) * 40).astype(np.float32)
        base = proto[rng.integers(0, 50, n)] + rng.standard_normal((n, d)).astype(np.float32) * np.float32(2e-3)
    else:
        lo, hi = RANGE[dtype]
        proto = rng.integers(lo + 1, hi, size=(50, d)).astype(np.float32)
        base = proto[rng.integers(0, 50, n)] + rng.integers(-1, 2, size=(n, d)).astype(np.float32)
    q = (proto[rng.integers(0, 50, nq)] + rng.standard_normal((nq, d)).astype(np.float32) * np.float32(0.3)).astype(np.float32)
    return widened(base.astype(np.float32), dtype), q


class Pair:
    """the narrow store under test and the fp32 store of the same (widened) rows"""

    def __init__(self, W, dtype, small_path=None, dist_budget=None):
        self.W = W
        self.g = api.GammaHip(0)
        self.g32 = api.GammaHip(0)
        d = W.shape[1]
        self.g.raw_init(d, dtype)
        self.g.set_flat_narrow_rows(True)
        self.g32.raw_init(d)
        for h in (self.g, self.g32):
            h.raw_append(W)
            if small_path is not None:
                h.set_small_path(small_path)
            if dist_budget is not None:
                h.set_dist_budget(dist_budget)
        assert self.g.raw_elem_type() == 1 + DTYPES.index(dtype) and self.g32.raw_elem_type() == 0

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


# ---- the switch -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_switch_turns_flat_search_over_narrow_rows_on(dtype):
    """off (the default): EUNSUPPORTED with the store's refusal message, as before; on: served; off again: refused again.
    With the switch on, raw_put and the IVFFLAT search still refuse the store."""
    d, N = 24, 700
    W = random_rows(N, d, dtype, 1)
    q = random_queries(8, d, dtype, 2)
    word = b"float16" if dtype == "float16" else b"8-bit"
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
        assert rc == EUNSUPPORTED and word in msg and what in msg, (rc, msg)

    try:
        g.raw_init(d, dtype)
        g.raw_append(W)
        refused(flat())
        g.set_flat_narrow_rows(True)
        assert flat() == 0
        Do, Io = B.flat_search(W, q, 5, B.METRIC_L2, B.make_ctx(**WIDE))
        compare_exact(Do, Io, D, I)
        vids = np.arange(4, dtype=np.int64)
        refused(L.gamma_hip_raw_put(g.h, 4, vids.ctypes.data_as(_lib.i64p), W[:4].ctypes.data_as(_lib.f32p)),
                b"gamma_hip_raw_init_")      # (the store's own message: rows sharded with their lists are fp32)
        g.set_flat_narrow_rows(False)
        refused(flat())
    finally:
        g.close()
    g = api.GammaHip(0)
    L = g.L
    try:
        cc = np.ascontiguousarray(W[:4])
        g.ivfflat_init(d, 4, api.METRIC_L2)
        g.ivfflat_set_trained(cc)
        g.raw_init(d, dtype)
        g.set_flat_narrow_rows(True)
        g.raw_append(W[:500])
        g.add_keys_batch([0], [500], np.arange(500), np.zeros((500, 1), np.uint8))
        refused(L.gamma_hip_ivfflat_search(g.h, args.ref(), 8, q.ctypes.data_as(_lib.f32p), 5, D.ctypes.data_as(_lib.f32p),
                                           I.ctypes.data_as(_lib.i64p)))
    finally:
        g.close()


def test_switch_leaves_an_fp32_store_alone():
    d, N = 32, 900
    W = random_rows(N, d, "int8", 3)
    q = random_queries(8, d, "int8", 4)
    g = api.GammaHip(0)
    try:
        g.raw_init(d)
        g.raw_append(W)
        r0 = g.flat_search(q, 5, api.SearchArgs(metric=api.METRIC_L2, **WIDE))
        g.set_flat_narrow_rows(True)
        r1 = g.flat_search(q, 5, api.SearchArgs(metric=api.METRIC_L2, **WIDE))
        assert r0[0].tobytes() == r1[0].tobytes() and r0[1].tobytes() == r1[1].tobytes()
    finally:
        g.close()


# ---- the slab kernels (kernels.hip) -----------------------------------------------------------------------------------
# N = 3001: a partial block of 128 (k_pairwise_lds) and of 256 rows (k_pairwise_rowreg / _generic).  nq = 16 goes to
# k_pairwise_lds for d in {128, 96, 64, 32, 16} (two threads per row, 16-byte loads) and to k_pairwise_generic otherwise: d = 20
# (byte rows aligned to 4 bytes, half rows to 8), d = 33 (rows aligned to their element only).  nq = 5: fewer than 8 queries per
# workgroup, so launch_pairwise_t sends the same d to k_pairwise_rowreg.
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d,nq", [(128, 16), (96, 16), (16, 16), (20, 16), (33, 16), (64, 5), (16, 5)])
def test_slab_kernels_over_narrow_rows(dtype, d, nq):
    N = 3001
    W = random_rows(N, d, dtype, 10 + d)
    q = random_queries(nq, d, dtype, 11 + d)
    rng = np.random.default_rng(d)
    bm = bitmap_of(N, rng.choice(N, N // 9, replace=False))
    docs = rng.choice(N, 3 * N // 4, replace=False)
    for small_path in (1, 0):   # one row chunk + the small tail | the chunked path (one chunk, no bound at this N)
        p = Pair(W, dtype, small_path=small_path)
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


@pytest.mark.parametrize("dtype", DTYPES)
def test_emitting_kernel_over_narrow_rows(dtype):
    """d = 16 has no matrix variant: the first chunk is 65536 rows, the remaining 4464 go through k_pairwise_lds<.., EMIT>
    under the running bound (24 queries: the small path is switched off)"""
    d, N, nq = 16, 70000, 24
    W = random_rows(N, d, dtype, 21)
    q = random_queries(nq, d, dtype, 22)
    p = Pair(W, dtype, small_path=0)
    try:
        for metric in METRICS:
            p.check(q, 10, metric)
    finally:
        p.close()


# ---- the matrix-pipe filter (flat_mfma.hip) ---------------------------------------------------------------------------
# nq = 96: more than the small path's 64 queries, and a padded tile of 64.  N = 21000: the first chunk is 16384 rows, then ONE
# pass of 4616 rows with a partial block of 128.
@pytest.mark.parametrize("dtype,kind", [("float16", "near_duplicates"), ("float16", "unit"), ("uint8", "near_duplicates"),
                                        ("int8", "near_duplicates")])
@pytest.mark.parametrize("d", [32, 128])
def test_matrix_filter_over_narrow_rows_never_drops_a_neighbour(dtype, kind, d):
    N, nq = 21000, 96
    W, q = margin_rows(N, d, dtype, kind, 100 + d, nq)
    rng = np.random.default_rng(d)
    bm = bitmap_of(N, rng.choice(N, N // 11, replace=False))
    docs = rng.choice(N, 3 * N // 4, replace=False)
    p = Pair(W, dtype)
    try:
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


@pytest.mark.parametrize("dtype,kind", [("float16", "near_duplicates"), ("float16", "unit"), ("uint8", "near_duplicates"),
                                        ("int8", "near_duplicates")])
@pytest.mark.parametrize("d", [160, 1056])
def test_long_row_filter_over_narrow_rows(dtype, kind, d):
    """k_flat_filter_big: d = 160 (the image in LDS) and d = 1056 (the LO_L2 form); a first chunk of 1024 rows, then passes of
    3072 and 904 rows"""
    N, nq = 5000, 96
    W, q = margin_rows(N, d, dtype, kind, 200 + d, nq)
    p = Pair(W, dtype)
    try:
        for metric in METRICS:
            p.check(q, 10, metric)
    finally:
        p.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("metric", METRICS, ids=["l2", "ip"])
def test_overflow_redo_reads_narrow_rows(dtype, metric):
    """Rows in improving order for query 0: every row of the pass behind the first chunk beats the bound, the query's list
    (2048 items) overflows and the call is redone without a bound -- two row chunks through one slab, so the tie phase
    recomputes the flagged queries' rows (the redo branch of tie_phase).  Every distinct row occurs about 14 times, so every
    query has exact ties among its best.  That the list must overflow is shown on the CPU (all 4616 rows of the pass are within
    the bound, against a capacity of 2048); the handle exposes no counter of redone calls, so that the redo ran is implied by
    that argument and not observed -- the test below reaches the same recompute branch by construction."""
    N, d, nq, k = 21000, 32, 96, 10
    W, q = margin_rows(1500, d, dtype, "near_duplicates", 300, nq)
    W = W[np.random.default_rng(7).integers(0, len(W), N)]      # every distinct row about 14 times: ties for every query

    def score(W):      # smaller is better
        if metric == B.METRIC_L2:
            return ((W.astype(np.float64) - q[0].astype(np.float64)) ** 2).sum(1)
        return -(W.astype(np.float64) @ q[0].astype(np.float64))

    W = np.ascontiguousarray(W[np.argsort(-score(W), kind="stable")])
    s0 = score(W)
    bound = np.sort(s0[:16384])[k]      # (k + 1 results are kept with exact ties on)
    assert int((s0[16384:] <= bound).sum()) > 2048
    p = Pair(W, dtype)
    try:
        D, I = p.check(q, k, metric)
        assert (D[:, 0] == D[:, 1]).all()      # ties among the results: the tie phase had every query to replay
    finally:
        p.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_tie_recompute_over_several_chunks_reads_narrow_rows(dtype):
    """d = 20 has neither an emitting kernel nor a matrix variant, so 70000 rows go through one slab as two row chunks without a
    bound, and every query with a tie has its rows computed again by the tie phase (launch_pairwise_filtered over the whole
    store, k_pairwise_generic).  Every distinct row occurs about 35 times: every query is such a query."""
    N, d, nq, k = 70000, 20, 24, 10
    W = random_rows(2000, d, dtype, 41)
    W = np.ascontiguousarray(W[np.random.default_rng(8).integers(0, len(W), N)])
    q = random_queries(nq, d, dtype, 42)
    p = Pair(W, dtype, small_path=0)
    try:
        for metric in METRICS:
            D, I = p.check(q, k, metric)
            assert (D[:, 0] == D[:, 1]).all()
    finally:
        p.close()
