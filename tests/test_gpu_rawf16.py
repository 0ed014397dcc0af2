"""GPU: the float16 raw store (gamma_hip_raw_init_f16) through api.GammaHip.

The conversion is compared bit for bit with numpy's float32 -> float16 (round to nearest even, subnormal halves kept).
Searches are compared strictly -- labels and distance bits at every rank, coarse and recall stage included, no query
excluded, exact ties on unless stated -- with the CPU oracle that `add`s the fp32 base and is given the ROUNDED rows as its
raw store (set_raw): only the store is rounded, so that oracle is the complete expected result.  The data is Gaussian x 3:
data that fp16 changes (integers <= 255 are exact in fp16 and would show nothing)."""
import numpy as np
import pytest

from gamma_amd import _lib, api
from oracle import binding as B
from tests import opq_ref as OR
from tests import pq4_ref as PR
from tests.parity import compare_exact, compare_search_exact

pytestmark = pytest.mark.gpu

N = 6000
WIDE = dict(min_score=-3e38, max_score=3e38)
EINVAL, EUNSUPPORTED = -1, -6   # include/gamma_hip.h
_cases = {}


def rounded(x):
    return np.ascontiguousarray(x, dtype=np.float32).astype(np.float16).astype(np.float32)


def gauss3(n, d, seed):
    return (3.0 * np.random.default_rng(seed).standard_normal((n, d))).astype(np.float32)


def _new_oracle(c):
    o = B.OracleIVFPQ(c["d"], c["nlist"], c["M"], 8, c["metric"])
    o.set_trained(c["cc"], c["pq"], None)
    B.lib().go_set_assign_mode(0)
    assert o.add(c["base"])
    return o


def _case(d, M, metric, nlist=16, base=None, tag=""):
    """base, its rounded rows, queries, the oracle's trained state and the oracle over the fp32 base (built once per shape,
    left unchanged: its raw store is switched between the rounded and the fp32 rows by the tests that need both)"""
    key = (d, M, metric, nlist, tag)
    if key not in _cases:
        if base is None:
            base = gauss3(N, d, 100 + d)
        cc, pq = B.ivfpq_train(base[:3000], nlist, M)
        c = dict(d=d, M=M, metric=metric, nlist=nlist, base=base, half=rounded(base), q=gauss3(300, d, 7 + d), cc=cc, pq=pq)
        c["oracle"] = _new_oracle(c)
        c["oracle"].set_raw(c["half"])
        _cases[key] = c
    return _cases[key]


def _handle(c, dtype="float16", o=None):
    """a handle holding exactly the oracle's lists, and the fp32 base handed to a raw store of the given element type"""
    o = o or c["oracle"]
    g = api.GammaHip(0)
    g.ivfpq_init(c["d"], c["nlist"], c["M"], 8, c["metric"])
    g.ivfpq_set_trained(c["cc"], c["pq"], None)
    lists, counts, vids, codes = [], [], [], []
    for l in range(c["nlist"]):
        ids, cds = o.get_list(l)
        if len(ids):
            lists.append(l)
            counts.append(len(ids))
            vids.append(ids)
            codes.append(cds)
    g.add_keys_batch(lists, counts, np.concatenate(vids), np.concatenate(codes))
    g.raw_init(c["d"], dtype)
    g.raw_append(c["base"])
    return g


def _check(g, o, q, k, P, R, metric, has_rank=True, exact_ties=0, ctx_kw=None, arg_kw=None, lo=-3e38, hi=3e38):
    ctx = B.make_ctx(min_score=lo, max_score=hi, **(ctx_kw or {}))
    D, I, st = o.search(q, k, P, recall_num=R, has_rank=has_rank, metric=metric, ctx=ctx, want_stages=True)
    args = api.SearchArgs(metric=metric, nprobe=P, recall_num=R, has_rank=has_rank, min_score=lo, max_score=hi,
                          exact_ties=exact_ties, **(arg_kw or {}))
    Dg, Ig = g.ivfpq_search(q, k, args)
    sg = g.last_stages(len(q), P, max(R, k))
    compare_search_exact(D, I, st, Dg, Ig, sg)
    return D, I


# ---- conversion -----------------------------------------------------------------------------------------------------
SPECIAL = np.array([6e-8, 2.9802325e-8, 2.98e-8, 1.0004883, 1.0014648, 65504.0, 65519.996, -6e-8, -65519.996, 0.0, -0.0,
                    5.9604645e-8, 6.1035156e-5, 6.0975552e-5, 0.1, -1e-3], dtype=np.float32)


@pytest.mark.parametrize("d", [1, 15, 20, 128])
def test_conversion_bits_and_writers(d):
    rng = np.random.default_rng(d)
    g = api.GammaHip(0)
    try:
        g.raw_init(d, "float16")
        assert g.raw_elem_bytes() == 2
        rows = 3.0 * rng.standard_normal((700, d)).astype(np.float32)
        flat = rows.reshape(-1)
        flat[:len(SPECIAL)] = SPECIAL            # the contract's cases, wherever they fall in a row
        flat[len(SPECIAL):2 * len(SPECIAL)] = -SPECIAL
        # the stated roundings, spelled out (numpy is the definition; these pin what it is expected to say)
        h = rounded(SPECIAL)
        assert h[2] == 0.0 and h[0] == np.float32(2.0 ** -24) and h[1] == np.float32(2.0 ** -24)
        assert h[3] == 1.0 and h[4] == np.float32(1.0019531) and h[5] == 65504.0 and h[6] == 65504.0
        g.raw_append(rows[:100])
        g.raw_append(rows[100:101])
        g.raw_append(rows[101:700])
        assert g.raw_count() == 700
        assert g.raw_gets(np.arange(700)).tobytes() == rounded(rows).tobytes()
        # raw_write (idempotent, may extend), raw_update, raw_update_batch (a vid named twice: the last wins; one beyond
        # the store: skipped)
        more = 3.0 * rng.standard_normal((40, d)).astype(np.float32)
        g.raw_write(690, more)
        rows = np.concatenate([rows[:690], more])
        assert g.raw_count() == 730
        g.raw_update(5, np.resize(SPECIAL, d))
        rows[5] = np.resize(SPECIAL, d)
        uv = np.array([3, 729, 17, 3, 100000], dtype=np.int64)
        ux = 3.0 * rng.standard_normal((5, d)).astype(np.float32)
        g.raw_update_batch(uv, ux)
        rows[729], rows[17], rows[3] = ux[1], ux[2], ux[3]
        assert g.raw_gets(np.arange(730)).tobytes() == rounded(rows).tobytes()
        assert g.total_mem_bytes() >= 730 * d * 2
        g.raw_clear()
        assert g.raw_count() == 0 and g.raw_elem_bytes() == 2
        g.raw_append(rows[:10])
        assert g.raw_gets(np.arange(10)).tobytes() == rounded(rows[:10]).tobytes()
    finally:
        g.close()


@pytest.mark.parametrize("in_place", [True, False], ids=["mapped", "reallocating"])
def test_three_appends_across_a_capacity_growth(in_place, monkeypatch):
    """rows of 2 * d bytes through the store's growth machinery: the mapped range grows by chunks of 64 MB (262144 rows of
    d = 128), the reallocating store (GAMMA_HIP_NO_RAW_VMM) from 1024 rows; the second append crosses the capacity"""
    d = 128
    if not in_place:
        monkeypatch.setenv("GAMMA_HIP_NO_RAW_VMM", "1")
    n0 = 262000 if in_place else 1000
    rows = gauss3(n0 + 300 + 100, d, 11)
    g = api.GammaHip(0)
    try:
        g.raw_init(d, "float16")
        g.raw_append(rows[:n0])
        st0 = g.raw_stats()
        assert not (st0["in_place"] and not in_place)
        in_place = st0["in_place"]            # (a runtime without virtual memory management: the store reallocates)
        assert st0["capacity"] < n0 + 300
        g.raw_append(rows[n0:n0 + 300])
        g.raw_append(rows[n0 + 300:])
        st = g.raw_stats()
        assert st["rows"] == len(rows) and st["capacity"] > st0["capacity"]
        assert st["moves"] == (0 if in_place else st0["moves"] + 1)
        assert g.total_mem_bytes() == st["capacity"] * d * 2
        sel = np.concatenate([np.arange(0, n0, 997), np.arange(n0 - 5, len(rows))])
        assert g.raw_gets(sel).tobytes() == rounded(rows[sel]).tobytes()
    finally:
        g.close()


def test_nonfinite_values_are_stored_as_they_convert():
    g = api.GammaHip(0)
    try:
        g.raw_init(4, "float16")
        x = np.array([[np.inf, -np.inf, np.nan, 1.0]], dtype=np.float32)
        g.raw_append(x)
        out = g.raw_gets([0])
        assert out[0, 0] == np.inf and out[0, 1] == -np.inf and np.isnan(out[0, 2]) and out[0, 3] == 1.0
    finally:
        g.close()


@pytest.mark.parametrize("bad", [65520.0, 70000.0, -65520.0])
def test_overflow_is_refused_before_anything_changes(bad):
    g = api.GammaHip(0)
    try:
        d = 20
        g.raw_init(d, "float16")
        rows = gauss3(50, d, 1)
        g.raw_append(rows)
        before = g.raw_stats()
        x = gauss3(30, d, 2)
        x[17, 3] = bad
        p = lambda a: a.ctypes.data_as(_lib.f32p)
        vids = np.arange(10, 40, dtype=np.int64)
        calls = [lambda: g.L.gamma_hip_raw_append(g.h, 30, p(x)),
                 lambda: g.L.gamma_hip_raw_write(g.h, 40, 30, p(x)),
                 lambda: g.L.gamma_hip_raw_update(g.h, 7, p(x[17])),
                 lambda: g.L.gamma_hip_raw_update_batch(g.h, 30, vids.ctypes.data_as(_lib.i64p), p(x))]
        for call in calls:
            assert call() == EINVAL
            assert b"float16" in g.L.gamma_hip_last_error(g.h)
            assert g.raw_stats() == before and g.raw_count() == 50
            assert g.raw_gets(np.arange(50)).tobytes() == rounded(rows).tobytes()
    finally:
        g.close()


# ---- search parity against the oracle with rounded rows ------------------------------------------------------------
SHAPES = [(128, 16), (96, 12), (20, 5), (15, 5)]   # d % 8: 0, 0, 4, 7 (odd d: rows aligned to 2 bytes only)


@pytest.mark.parametrize("metric", [api.METRIC_L2, api.METRIC_IP], ids=["l2", "ip"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "d%d_m%d" % s)
def test_search_parity(shape, metric):
    d, M = shape
    c = _case(d, M, metric)
    g = _handle(c)
    try:
        for nq in (1, 8, 300):
            for R in (32, 200):
                _check(g, c["oracle"], c["q"][:nq], 10, 8, R, metric)
        assert g.ties_not_honoured() == 0
    finally:
        g.close()


def test_the_stores_can_be_told_apart():
    """the expected distances over the rounded rows differ in bits from those over the fp32 rows, and a handle with an
    fp32 store (the new getter says 4 bytes) equals the oracle on fp32 rows"""
    c = _case(128, 16, api.METRIC_L2)
    o = c["oracle"]
    q = c["q"][:64]
    ctx = B.make_ctx(**WIDE)
    Dh, Ih = o.search(q, 10, 8, recall_num=200, has_rank=True, metric=c["metric"], ctx=ctx)
    o.set_raw(c["base"])
    try:
        D32, I32 = o.search(q, 10, 8, recall_num=200, has_rank=True, metric=c["metric"], ctx=ctx)
        assert Dh.tobytes() != D32.tobytes()
        assert (Dh.view(np.uint32) != D32.view(np.uint32)).mean() > 0.5
        g = _handle(c, dtype="float32")
        try:
            assert g.raw_elem_bytes() == 4
            _check(g, o, q, 10, 8, 200, c["metric"])
        finally:
            g.close()
    finally:
        o.set_raw(c["half"])
    g = _handle(c)
    try:
        args = api.SearchArgs(metric=c["metric"], nprobe=8, recall_num=200, has_rank=True, **WIDE)
        Dg, Ig = g.ivfpq_search(q, 10, args)
        compare_exact(Dh, Ih, Dg, Ig)
    finally:
        g.close()


def test_recall_num_beyond_the_fused_kernel():
    """recall_num 1100: launch_rerank_dist over half rows, the selection, the tie flags made afterwards"""
    for d, M in ((128, 16), (15, 5)):
        c = _case(d, M, api.METRIC_L2)
        g = _handle(c)
        try:
            _check(g, c["oracle"], c["q"][:40], 10, 8, 1100, c["metric"])
        finally:
            g.close()


def test_unfused_path_without_exact_ties():
    """nq = 100 with exact ties off for the request: k_rerank_dist + selection (Gaussian data: no ties to honour)"""
    for d, M, metric in ((96, 12, api.METRIC_IP), (20, 5, api.METRIC_L2), (15, 5, api.METRIC_IP)):
        c = _case(d, M, metric)
        g = _handle(c)
        try:
            _check(g, c["oracle"], c["q"][:100], 10, 8, 200, metric, exact_ties=-1)
        finally:
            g.close()


def test_without_rank_equals_the_fp32_store():
    c = _case(96, 12, api.METRIC_L2)
    gh, gf = _handle(c), _handle(c, dtype="float32")
    try:
        for nq in (8, 300):
            q = c["q"][:nq]
            _check(gh, c["oracle"], q, 10, 8, 200, c["metric"], has_rank=False)
            args = api.SearchArgs(metric=c["metric"], nprobe=8, recall_num=200, has_rank=False, **WIDE)
            Dh, Ih = gh.ivfpq_search(q, 10, args)
            Df, If = gf.ivfpq_search(q, 10, args)
            assert Dh.tobytes() == Df.tobytes() and np.array_equal(Ih, If)
    finally:
        gh.close()
        gf.close()


def test_score_window():
    for d, M, metric in ((128, 16, api.METRIC_L2), (20, 5, api.METRIC_IP)):
        c = _case(d, M, metric)
        g = _handle(c)
        try:
            q = c["q"][:300]
            D, _ = _check(g, c["oracle"], q, 10, 8, 200, metric)
            lo, hi = sorted((float(np.median(D[:, 2])), float(np.median(D[:, 7]))))
            _check(g, c["oracle"], q, 10, 8, 200, metric, lo=lo, hi=hi)
            _check(g, c["oracle"], q[:8], 10, 8, 200, metric, lo=lo, hi=hi)
        finally:
            g.close()


def test_deleted_docs_and_range_filter():
    c = _case(96, 12, api.METRIC_L2)
    rng = np.random.default_rng(3)
    dead = rng.choice(N, N // 10, replace=False)
    bm = np.zeros(N // 8 + 1, np.uint8)
    np.bitwise_or.at(bm, dead >> 3, (1 << (dead & 7)).astype(np.uint8))
    allowed = np.nonzero(rng.random(N) < 0.6)[0]
    g = _handle(c)
    try:
        g.bitmap_upload(bm, N)
        for nq in (8, 300):
            _check(g, c["oracle"], c["q"][:nq], 10, 8, 200, c["metric"],
                   ctx_kw=dict(docids_bitmap=bm, range_filters=[B.make_range_filter(allowed)]),
                   arg_kw=dict(range_filters=[api.make_range_filter(allowed)]))
    finally:
        g.close()


# ---- ties that exist only in the half store -----------------------------------------------------------------------
def _twins(d):
    a = gauss3(N // 2, d, 500 + d)
    base = np.concatenate([a, a * np.float32(1 + 2.0 ** -16)])
    return np.ascontiguousarray(base[np.random.default_rng(9).permutation(N)])


@pytest.mark.parametrize("d,M,metric", [(16, 4, api.METRIC_L2), (24, 6, api.METRIC_IP)], ids=["d16_l2", "d24_ip"])
def test_ties_of_the_rounded_rows_are_replayed(d, M, metric):
    """3000 rows and their twins row * (1 + 2^-16): distinct in fp32, mostly equal after rounding -- nearly every query has
    equal neighbouring exact distances on the half store and hardly any on fp32 rows; their order is the reference heaps'"""
    import torch
    base = _twins(d)
    assert len(np.unique(base, axis=0)) == N and len(np.unique(rounded(base), axis=0)) < N * 3 // 4
    c = _case(d, M, metric, base=base, tag="twins")
    o = c["oracle"]
    q, k, P, R = c["q"], 10, 8, 100
    ctx = B.make_ctx(**WIDE)
    D, I = o.search(q, k, P, recall_num=R, has_rank=True, metric=metric, ctx=ctx)
    assert (D[:, 1:] == D[:, :-1]).any(axis=1).mean() > 0.9          # ties on the rounded rows ...
    o.set_raw(c["base"])
    try:
        D32, _ = o.search(q, k, P, recall_num=R, has_rank=True, metric=metric, ctx=ctx)
    finally:
        o.set_raw(c["half"])
    assert (D32[:, 1:] == D32[:, :-1]).any(axis=1).mean() < 0.1      # ... that the fp32 rows do not have
    g = _handle(c)
    try:
        for nq in (300, 8):
            g.tie_stats(reset=True)
            _check(g, o, q[:nq], k, P, R, metric)
            assert g.tie_stats()["replayed"] > 0
        # the deferred replay on the side stream, through the _wait entry
        dev = torch.device("cuda", 0)
        tq = torch.from_numpy(q).to(dev)
        tD = torch.empty((len(q), k), dtype=torch.float32, device=dev)
        tI = torch.empty((len(q), k), dtype=torch.int64, device=dev)
        args = api.SearchArgs(metric=metric, nprobe=P, recall_num=R, has_rank=True, **WIDE)
        g.set_deferred_replay(True)
        g.tie_stats(reset=True)
        g.ivfpq_search_device_wait(tq.data_ptr(), len(q), k, args, tD.data_ptr(), tI.data_ptr())
        compare_exact(D, I, tD.cpu().numpy(), tI.cpu().numpy())
        assert g.tie_stats()["replayed"] > 0
        g.set_deferred_replay(False)
        assert g.ties_not_honoured() == 0
    finally:
        g.close()


# ---- other handles ------------------------------------------------------------------------------------------------
def test_four_bit_handle():
    d, nlist, M = 32, 16, 8
    base = gauss3(N, d, 41)
    cc, pq = PR.train(base[:3000], nlist, M)
    B.lib().go_set_assign_mode(-1)
    lno, codes = PR.encode(base, cc, pq)
    ix = PR.Index(cc, pq, PR.build_lists(lno, codes, nlist), raw=rounded(base))
    g = api.GammaHip(0)
    try:
        g.ivfpq4_init(d, nlist, M, api.METRIC_L2)
        g.ivfpq_set_trained(cc, pq, None)
        g.raw_init(d, "float16")
        g.raw_append(base)
        g.add(base, 0)
        q = gauss3(300, d, 42)
        for nq in (8, 300):
            args = api.SearchArgs(metric=api.METRIC_L2, nprobe=8, recall_num=100, has_rank=True, **WIDE)
            Dg, Ig = g.ivfpq_search(q[:nq], 10, args)
            sg = g.last_stages(nq, 8, 100)
            D, I, st = ix.search(q[:nq], 10, 8, recall_num=100, has_rank=True, l2=True, min_score=-3e38, max_score=3e38)
            compare_search_exact(D, I, st, Dg, Ig, sg)
    finally:
        g.close()


def test_handle_with_an_opq_matrix():
    d, nlist, M, metric = 32, 16, 8, api.METRIC_L2
    A = OR.random_rotation(d, 100 + d)
    base = gauss3(N, d, 51)
    half = rounded(base)

    def empty():
        g = api.GammaHip(0)
        g.ivfpq_init(d, nlist, M, 8, metric)
        g.opq_set(A)
        return g

    g = empty()
    try:
        base_rot = g.opq_apply(base)
        o, cc, pq = OR.build_oracle(base_rot, nlist, M, metric)
        g.ivfpq_set_trained(cc, pq, None)
        g.raw_init(d, "float16")
        g.raw_append(base)
        g.add(base, 0)
        for nq, R in ((8, 50), (300, 50)):
            q = OR.pick_queries(o, half, A, gauss3(nq + 40, d, 52), nq, 10, 8, R, metric)
            q_rot = g.opq_apply(q)
            D, I, st = OR.search_ref(o, half, q, q_rot, 10, 8, R, True, metric, min_score=-3e38, max_score=3e38)
            args = api.SearchArgs(metric=metric, nprobe=8, recall_num=R, has_rank=True, **WIDE)
            Dg, Ig = g.ivfpq_search(q, 10, args)
            compare_search_exact(D, I, st, Dg, Ig, g.last_stages(nq, 8, R))
    finally:
        g.close()


# ---- realtime -----------------------------------------------------------------------------------------------------
def test_update_batch_rewrites_the_rows():
    c = _case(20, 5, api.METRIC_L2)
    o = _new_oracle(c)                     # this test changes its oracle
    raw = c["half"].copy()
    g = _handle(c, o=o)
    try:
        rng = np.random.default_rng(12)
        vids = rng.choice(N, 50, replace=False).astype(np.int64)
        vecs = gauss3(50, c["d"], 77)
        g.update_batch(vids, vecs)
        g.raw_update_batch(vids, vecs)
        B.lib().go_set_assign_mode(-1)
        try:
            for v, x in zip(vids, vecs):
                o.update(int(v), x)
        finally:
            B.lib().go_set_assign_mode(0)
        raw[vids] = rounded(vecs)
        o.set_raw(raw)
        for l in range(c["nlist"]):
            ids, cds = g.get_list(l)
            oi, oc = o.get_list(l)
            assert np.array_equal(ids, oi) and cds.tobytes() == oc.tobytes(), "list %d after Update" % l
        for nq in (8, 300):
            _check(g, o, c["q"][:nq], 10, 8, 200, c["metric"])
        # an Add behind it: rows and keys of new vectors
        extra = gauss3(64, c["d"], 78)
        g.raw_append(extra)
        g.add(extra, N)
        B.lib().go_set_assign_mode(1)
        try:
            assert o.add(extra)
        finally:
            B.lib().go_set_assign_mode(0)
        o.set_raw(np.concatenate([raw, rounded(extra)]))
        _check(g, o, c["q"][:300], 10, 8, 200, c["metric"])
    finally:
        g.close()


# ---- refusals -----------------------------------------------------------------------------------------------------
def test_readers_of_fp32_rows_refuse_the_half_store():
    import torch
    c = _case(20, 5, api.METRIC_L2)
    g = _handle(c)
    L = g.L
    eunsup = EUNSUPPORTED

    def refused(rc):
        msg = L.gamma_hip_last_error(g.h)
        assert rc == eunsup and b"float16" in msg, (rc, msg)

    try:
        q = c["q"][:8]
        args = api.SearchArgs(metric=c["metric"], nprobe=8, recall_num=50, has_rank=True, **WIDE)
        D = np.empty((8, 10), np.float32)
        I = np.empty((8, 10), np.int64)
        refused(L.gamma_hip_flat_search(g.h, args.ref(), 8, q.ctypes.data_as(_lib.f32p), 10, D.ctypes.data_as(_lib.f32p),
                                        I.ctypes.data_as(_lib.i64p)))
        vids = np.arange(4, dtype=np.int64)
        refused(L.gamma_hip_raw_put(g.h, 4, vids.ctypes.data_as(_lib.i64p), c["base"][:4].ctypes.data_as(_lib.f32p)))
        refused(L.gamma_hip_raw_drop(g.h, 4, vids.ctypes.data_as(_lib.i64p)))
        tq = torch.from_numpy(q).cuda()
        tids = torch.zeros((8, 50), dtype=torch.int64, device="cuda")
        tex = torch.empty((8, 50), dtype=torch.float32, device="cuda")
        refused(L.gamma_hip_ivfpq_shard_exact(g.h, args.ref(), 8, tq.data_ptr(), tids.data_ptr(), 50, tex.data_ptr()))
    finally:
        g.close()
    g = api.GammaHip(0)
    try:
        g.ivfflat_init(c["d"], c["nlist"], c["metric"])
        g.ivfflat_set_trained(c["cc"])
        g.raw_init(c["d"], "float16")
        g.raw_append(c["base"][:500])
        g.add_keys_batch([0], [500], np.arange(500), np.zeros((500, 1), np.uint8))
        rc = L.gamma_hip_ivfflat_search(g.h, args.ref(), 8, q.ctypes.data_as(_lib.f32p), 10, D.ctypes.data_as(_lib.f32p),
                                        I.ctypes.data_as(_lib.i64p))
        refused(rc)
    finally:
        g.close()


def test_element_type_is_fixed_at_init():
    g = api.GammaHip(0)
    try:
        assert g.raw_elem_bytes() == 0
        g.raw_init(8, "float16")
        assert g.L.gamma_hip_raw_init(g.h, 8) == EINVAL
        assert g.L.gamma_hip_raw_init_f16(g.h, 8) == 0
        with pytest.raises(ValueError):
            g.raw_init(8, "bfloat16")
    finally:
        g.close()
