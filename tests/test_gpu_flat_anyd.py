"""GPU: the flat search's matrix-pipe filter for any row length 1 <= d <= 4096 (k_flat_filter_any).

The filter is a superset test and its survivors get the reference's arithmetic, so every result must be
  * the CPU oracle's exhaustive flat search, labels at every rank and distance bits, exact ties on (compare_exact), and
  * byte for byte what the SAME handle answers for the same queries in slices of 32 -- below the filter's gate of 64 queries,
    so scored exactly throughout.  The handles run with the small-batch path off: it takes calls of up to 64 queries in front
    of the chunked path, and 64 queries -- the gate itself, one padded tile -- is one of the batch sizes here.
That the filter ran is read from gamma_hip_flat_filter_stats: the (query, row) pairs its passes scored.

Shapes: N = 24001 rows for d <= 136 (a first chunk of 4096 / 16384 / 1024 rows, then passes whose last step of 256 rows is
partial), N = 6001 beyond (first chunk 1024 rows, passes of 3072 and 1905).  The lengths cover odd d (fp32 rows aligned to 4
bytes: element loads), d % 8 == 0 with d % 32 != 0 (wide loads, a masked tail), d < 32, just above 1536, 2500 (hi fragments
of the image in LDS, lo fragments partly in memory: the image's first 152 KB are resident, 2 * 2528 / 16 = 316 blocks) and
4096 (512 blocks: part of the hi fragments in memory too)."""
import numpy as np
import pytest

from gamma_amd import api
from oracle import binding as B
from tests.parity import compare_exact, compare_topk

pytestmark = pytest.mark.gpu

WIDE = dict(min_score=-3e38, max_score=3e38)
NP = {"float16": np.float16, "uint8": np.uint8, "int8": np.int8}
RANGE = {"uint8": (0, 255), "int8": (-128, 127)}
METRICS = (B.METRIC_L2, B.METRIC_IP)


def rows_for(d):
    return 24001 if d <= 136 else 6001


def first_chunk(d):
    """rows of the first, exactly scored chunk (flat_search_device_locked)"""
    if d > 128:
        return 1024
    return 16384 if d in (32, 64, 96, 128) else 4096


def passes_of(N, d):
    """(number of filter passes, rows they score): every pass scores 3 x the rows scored so far"""
    r, n = first_chunk(d), 0
    while r < N:
        r += min(3 * r, N - r)
        n += 1
    return n, N - first_chunk(d)


def make_data(kind, N, d, nq, seed):
    rng = np.random.default_rng(seed)
    if kind == "near_duplicates":      # thousands of distances within the margin of the k-th
        proto = (rng.standard_normal((50, d)) * 40).astype(np.float32)
        base = (proto[rng.integers(0, 50, N)] + rng.standard_normal((N, d)).astype(np.float32) * np.float32(2e-3)).astype(np.float32)
        q = (proto[rng.integers(0, 50, nq)] + rng.standard_normal((nq, d)).astype(np.float32) * np.float32(1e-3)).astype(np.float32)
    elif kind == "wide_range":         # columns over six decades
        scale = (10.0 ** rng.uniform(-3, 3, d)).astype(np.float32)
        base = (rng.standard_normal((N, d)).astype(np.float32) * scale).astype(np.float32)
        q = (rng.standard_normal((nq, d)).astype(np.float32) * scale).astype(np.float32)
    else:                              # unit vectors
        base = rng.standard_normal((N, d)).astype(np.float32)
        base /= np.linalg.norm(base, axis=1, keepdims=True)
        q = rng.standard_normal((nq, d)).astype(np.float32)
        q /= np.linalg.norm(q, axis=1, keepdims=True)
    return np.ascontiguousarray(base), np.ascontiguousarray(q)


def bitmap_of(n, dead):
    bm = np.zeros((n >> 3) + 1, dtype=np.uint8)
    np.bitwise_or.at(bm, dead >> 3, (1 << (dead & 7)).astype(np.uint8))
    return bm


def sliced(g, q, k, args):
    """the same handle, 32 queries at a time: the exact path"""
    parts = [g.flat_search(q[i:i + 32], k, args) for i in range(0, len(q), 32)]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def check(g, W, q, k, metric, win=WIDE, ctx_kw=None, kw=None, filtered=True, exact=True):
    """one call against the oracle and against the sliced calls; returns the pairs the filter scored in the call"""
    ctx_kw, kw = ctx_kw or {}, kw or {}
    D, I = B.flat_search(W, q, k, metric, B.make_ctx(**win, **ctx_kw))
    args = api.SearchArgs(metric=metric, **win, **kw)
    s0 = g.flat_filter_stats()
    Dg, Ig = g.flat_search(q, k, args)
    s1 = g.flat_filter_stats()
    Ds, Is = sliced(g, q, k, args)
    s2 = g.flat_filter_stats()
    assert s2 == s1, "a call of 32 queries went through the filter"
    if exact:
        compare_exact(D, I, Dg, Ig)
    else:
        compare_topk(D, I, Dg, Ig)
    assert Dg.tobytes() == Ds.tobytes() and Ig.tobytes() == Is.tobytes()
    if filtered:
        assert s1[0] > s0[0] and s1[1] > s0[1], (s0, s1)
    else:
        assert s1 == s0, (s0, s1)
    return s1[1] - s0[1], s1[0] - s0[0], s1[2] - s0[2]


# ---- 1. lengths -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["near_duplicates", "wide_range", "unit"])
@pytest.mark.parametrize("d", [24, 65, 100, 136, 300, 1000, 1537, 2048, 2500, 4096])
def test_any_length_filter_never_drops_a_neighbour(d, kind):
    N = rows_for(d)
    assert api.flat_filter_shape(d)[0] == (d + 31) // 32 * 32
    base, q = make_data(kind, N, d, 200, 1000 + d)
    rng = np.random.default_rng(d)
    bm = bitmap_of(N, rng.choice(N, N // 11, replace=False))
    docs = rng.choice(N, 3 * N // 4, replace=False)
    g = api.GammaHip(0)
    try:
        g.set_small_path(0)      # (a call of up to 64 queries would take the one-chunk path in front of the filter's gate)
        g.raw_init(d)
        g.raw_append(base)
        for step in range(2):
            ctx_kw, kw = {}, {}
            if step == 1:
                g.bitmap_upload(bm, N)
                ctx_kw = dict(docids_bitmap=bm, range_filters=[B.make_range_filter(docs)])
                kw = dict(range_filters=[api.make_range_filter(docs)])
            for metric in METRICS:
                for nq, k in ((64, 10), (200, 100), (130, 1)):
                    wins = [WIDE]
                    if step == 1 and k == 10:
                        Dw, _ = B.flat_search(base, q[:nq], k, metric, B.make_ctx(**WIDE, **ctx_kw))
                        wins.append(dict(min_score=float(np.quantile(Dw, 0.2)), max_score=float(np.quantile(Dw, 0.9))))
                    for win in wins:
                        pairs, passes, _ = check(g, base, q[:nq], k, metric, win, ctx_kw, kw)
                        # (a call redone without the bound has scored its pairs too: >=, and == when nothing was redone)
                        assert pairs >= nq * passes_of(N, d)[1]
    finally:
        g.close()


# ---- 2. narrow rows ---------------------------------------------------------------------------------------------------
def narrow_data(N, d, dtype, nq, seed):
    """rows on the filter's margin that the store of this type holds exactly: W = base.astype(T).astype(float32)"""
    rng = np.random.default_rng(seed)
    if dtype == "float16":
        proto = (rng.standard_normal((50, d)) * 40).astype(np.float32)
        base = proto[rng.integers(0, 50, N)] + rng.standard_normal((N, d)).astype(np.float32) * np.float32(2e-3)
    else:
        lo, hi = RANGE[dtype]
        proto = rng.integers(lo + 1, hi, size=(50, d)).astype(np.float32)
        base = proto[rng.integers(0, 50, N)] + rng.integers(-1, 2, size=(N, d)).astype(np.float32)
        base[0, 0], base[0, -1] = lo, hi
    q = (proto[rng.integers(0, 50, nq)] + rng.standard_normal((nq, d)).astype(np.float32) * np.float32(0.3)).astype(np.float32)
    W = np.ascontiguousarray(base.astype(np.float32).astype(NP[dtype]).astype(np.float32))
    return W, q


@pytest.mark.parametrize("dtype", ["float16", "uint8", "int8"])
@pytest.mark.parametrize("d", [100, 301, 2048])
def test_any_length_filter_over_narrow_rows(d, dtype):
    """d = 100: rows of 200 / 100 bytes (d % 8 != 0: element loads); 301: odd rows; 2048: the wide loads"""
    N, nq = 6001, 96
    W, q = narrow_data(N, d, dtype, nq, 2000 + d)
    g = api.GammaHip(0)
    try:
        g.set_small_path(0)      # (a call of up to 64 queries would take the one-chunk path in front of the filter's gate)
        g.raw_init(d, dtype)
        g.set_flat_narrow_rows(True)
        g.raw_append(W)
        for metric in METRICS:
            for k in (1, 10):
                check(g, W, q, k, metric)
    finally:
        g.close()


# ---- 3. ties ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [100, 2048])
def test_any_length_filter_with_exact_ties(d):
    """every distinct row four times: k = 10 cuts a group of equal distances.  exact_ties on: the reference heap's order and
    membership; off: the same distances at every rank, ids up to the order inside a tie"""
    N, nq, k = rows_for(d), 96, 10
    distinct, q = make_data("unit", N // 4 + 1, d, nq, 3000 + d)
    pick = np.arange(N) % len(distinct)
    np.random.default_rng(d).shuffle(pick)
    base = np.ascontiguousarray(distinct[pick])
    g = api.GammaHip(0)
    try:
        g.set_small_path(0)      # (a call of up to 64 queries would take the one-chunk path in front of the filter's gate)
        g.raw_init(d)
        g.raw_append(base)
        for metric in METRICS:
            check(g, base, q, k, metric)
        g.set_exact_ties(False)
        for metric in METRICS:
            check(g, base, q, k, metric, exact=False)
    finally:
        g.close()


# ---- 4. overflow ------------------------------------------------------------------------------------------------------
def test_survivor_list_overflow_is_redone_without_the_bound():
    """6001 rows that are copies of 8 distinct rows, the 8 within 2e-3 per element of ONE prototype of norm ~700: every row is
    within the margin (2^-12 (xn + yn) ~ 230) of every query's k-th best, so all 3072 rows of the first pass survive for all
    64 queries -- 196608 pairs against the pair list's 64 x 1024 -- and the call is redone without the bound"""
    d, N, nq, k = 300, 6001, 64, 10
    rng = np.random.default_rng(4000)
    proto = (rng.standard_normal((1, d)) * 40).astype(np.float32)
    distinct = (proto + rng.standard_normal((8, d)).astype(np.float32) * np.float32(2e-3)).astype(np.float32)
    q = (proto + rng.standard_normal((nq, d)).astype(np.float32) * np.float32(1e-3)).astype(np.float32)
    base = np.ascontiguousarray(distinct[np.random.default_rng(1).integers(0, 8, N)])
    g = api.GammaHip(0)
    try:
        g.set_small_path(0)      # (a call of up to 64 queries would take the one-chunk path in front of the filter's gate)
        g.raw_init(d)
        g.raw_append(base)
        for metric in METRICS:
            _, _, redone = check(g, base, q, k, metric)
            assert redone > 0
    finally:
        g.close()


# ---- 5. gates ---------------------------------------------------------------------------------------------------------
def test_gates_keep_small_calls_off_the_filter():
    d, N = 100, 24001
    base, q = make_data("unit", N, d, 64, 5000)
    g = api.GammaHip(0)
    try:
        g.set_small_path(0)      # (a call of up to 64 queries would take the one-chunk path in front of the filter's gate)
        g.raw_init(d)
        g.raw_append(base)
        check(g, base, q[:64], 257, B.METRIC_L2, filtered=False)
        check(g, base, q[:63], 10, B.METRIC_L2, filtered=False)
        check(g, base, q[:64], 10, B.METRIC_L2)
    finally:
        g.close()


# ---- 6. old shapes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [128, 768])
def test_old_shapes_score_exactly_the_pairs_they_scored(d):
    N, nq = rows_for(d), 200
    base, q = make_data("unit", N, d, nq, 6000 + d)
    g = api.GammaHip(0)
    try:
        g.set_small_path(0)      # (a call of up to 64 queries would take the one-chunk path in front of the filter's gate)
        g.raw_init(d)
        g.raw_append(base)
        npass, rows = passes_of(N, d)
        for metric in METRICS:
            pairs, passes, redone = check(g, base, q, 10, metric)
            assert (passes, pairs, redone) == (npass, nq * rows, 0)
    finally:
        g.close()


# ---- 7. plugin --------------------------------------------------------------------------------------------------------
def test_hipflat_plugin_at_d_100():
    """Add, Search, Delete, Search: 128 queries over 6000 rows of 100 floats (first chunk 4096 rows, one filter pass).
    A model keeps its handle to itself and the plugin interface has no counter, so this case cannot assert that the filter
    ran -- the shape is that of test_gates_keep_small_calls_off_the_filter's last call, which does; what it checks is that
    the model's Search reaches gamma_hip_flat_search with rows of 100 floats and answers what the oracle answers."""
    from gamma_amd import plugin
    d, N = 100, 6000
    base, q = make_data("near_duplicates", N, d, 128, 7000)
    for name, bmetric in (("L2", B.METRIC_L2), ("InnerProduct", B.METRIC_IP)):
        m = plugin.PluginModel("HIPFLAT", d, '{"metric_type": "%s"}' % name)
        try:
            m.store(base)
            assert m.add(base[:3000]) and m.add(base[3000:])
            D, I = B.flat_search(base, q, 10, bmetric, B.make_ctx())
            compare_exact(D, I, *m.search(q, 10, ""))
            dead = np.unique(I[:, :2])
            assert m.delete(dead) == 0
            bmap = np.zeros((N + 7) // 8, np.uint8)
            np.bitwise_or.at(bmap, dead >> 3, (1 << (dead & 7)).astype(np.uint8))
            D, I = B.flat_search(base, q, 10, bmetric, B.make_ctx(docids_bitmap=bmap))
            compare_exact(D, I, *m.search(q, 10, ""))
        finally:
            m.close()
