"""GPU: the 8-bit raw stores (gamma_hip_raw_init_i8: uint8 and int8 rows) through api.GammaHip.

The store is lossless or refuses: a byte widens to fp32 exactly, so the complete expected result is the CPU oracle over the
untouched fp32 base (the data has no -0.0), and a handle with a byte store answers byte for byte what a handle with an fp32
store holding the same lists answers.  Searches are compared strictly -- labels and distance bits at every rank, coarse and
recall stage included, no query and no rank excluded.  The data is integer-valued over the element type's whole range, both
extremes included: sums over such rows are not representable in fp16, so a store that rounded anywhere would show."""
import ctypes as C

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
RANGE = {"uint8": (0, 255), "int8": (-128, 127)}
ETYPE = {"uint8": 2, "int8": 3}
DTYPES = ["uint8", "int8"]
_trained, _cases = {}, {}


def ints(n, d, dtype, seed):
    """integer-valued fp32 rows over the whole range of the type; the first row holds both extremes"""
    lo, hi = RANGE[dtype]
    x = np.random.default_rng(seed).integers(lo, hi + 1, size=(n, d)).astype(np.float32)
    x[0, 0], x[0, -1] = lo, hi
    if d == 1:
        x[1, 0] = lo
    return x


def gauss(n, d, dtype, seed):
    """Gaussian fp32 queries around the middle of the type's range"""
    lo, hi = RANGE[dtype]
    return ((lo + hi) / 2.0 + 60.0 * np.random.default_rng(seed).standard_normal((n, d))).astype(np.float32)


def _new_oracle(c):
    o = B.OracleIVFPQ(c["d"], c["nlist"], c["M"], 8, c["metric"])
    o.set_trained(c["cc"], c["pq"], None)
    B.lib().go_set_assign_mode(0)
    assert o.add(c["base"])
    o.set_raw(c["base"])
    return o


def _case(d, M, metric, dtype, nlist=16, base=None, tag=""):
    """base, queries (Gaussian, and byte-valued ones), the trained state (once per shape and type) and the oracle over the fp32
    base (once per shape, type and metric; left unchanged)"""
    tkey = (d, M, dtype, nlist, tag)
    if tkey not in _trained:
        if base is None:
            base = ints(N, d, dtype, 100 + d)
        assert not np.signbit(base[base == 0]).any()          # no -0.0: the oracle over the untouched base is the reference
        cc, pq = B.ivfpq_train(base[:3000], nlist, M)
        _trained[tkey] = dict(d=d, M=M, nlist=nlist, dtype=dtype, base=base, q=gauss(300, d, dtype, 7 + d),
                              qb=ints(300, d, dtype, 9 + d), cc=cc, pq=pq)
    key = tkey + (metric,)
    if key not in _cases:
        c = dict(_trained[tkey], metric=metric)
        c["oracle"] = _new_oracle(c)
        _cases[key] = c
    return _cases[key]


def _handle(c, dtype=None, o=None):
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
    g.raw_init(c["d"], dtype or c["dtype"])
    g.raw_append(c["base"])
    return g


def _check(g, o, q, k, P, R, metric, has_rank=True, exact_ties=0, ctx_kw=None, arg_kw=None, lo=-3e38, hi=3e38, g32=None):
    """the handle against the oracle; with g32 (a handle with an fp32 store and the same lists) also byte for byte against it"""
    ctx = B.make_ctx(min_score=lo, max_score=hi, **(ctx_kw or {}))
    D, I, st = o.search(q, k, P, recall_num=R, has_rank=has_rank, metric=metric, ctx=ctx, want_stages=True)
    args = api.SearchArgs(metric=metric, nprobe=P, recall_num=R, has_rank=has_rank, min_score=lo, max_score=hi,
                          exact_ties=exact_ties, **(arg_kw or {}))
    Dg, Ig = g.ivfpq_search(q, k, args)
    sg = g.last_stages(len(q), P, max(R, k))
    compare_search_exact(D, I, st, Dg, Ig, sg)
    if g32 is not None:
        Df, If = g32.ivfpq_search(q, k, args)
        assert Dg.tobytes() == Df.tobytes() and Ig.tobytes() == If.tobytes()
    return D, I


def _mem(g):
    st = g.raw_stats()
    return st, g.total_mem_bytes()


# ---- conversion and writers ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [1, 15, 20, 128])
def test_conversion_and_writers(d, dtype):
    lo, hi = RANGE[dtype]
    g = api.GammaHip(0)
    try:
        assert g.raw_elem_type() == 0
        g.raw_init(d, dtype)
        assert g.raw_elem_bytes() == 1 and g.raw_elem_type() == ETYPE[dtype]
        rows = ints(700, d, dtype, d)
        flat = rows.reshape(-1)
        allv = np.arange(lo, hi + 1, dtype=np.float32)      # every value of the type, wherever it falls in a row
        flat[:256] = allv[:min(256, flat.size)]
        flat[300] = -0.0                                     # accepted, stored as 0
        g.raw_append(rows[:100])
        g.raw_append(rows[100:101])
        g.raw_append(rows[101:700])
        assert g.raw_count() == 700
        want = rows + np.float32(0.0)                        # (-0.0 + 0.0 = +0.0)
        got = g.raw_gets(np.arange(700))
        assert got.tobytes() == want.tobytes() and not np.signbit(got.reshape(-1)[300])
        # raw_write (idempotent, may extend), raw_update, raw_update_batch (a vid named twice: the last wins; one beyond the
        # store and a negative one: skipped)
        more = ints(40, d, dtype, d + 1)
        g.raw_write(690, more)
        rows = np.concatenate([want[:690], more])
        assert g.raw_count() == 730
        g.raw_update(5, np.resize(allv[::-1], d))
        rows[5] = np.resize(allv[::-1], d)
        uv = np.array([3, 729, 17, 3, 100000, -1], dtype=np.int64)
        ux = ints(6, d, dtype, d + 2)
        g.raw_update_batch(uv, ux)
        rows[729], rows[17], rows[3] = ux[1], ux[2], ux[3]
        assert g.raw_gets(np.arange(730)).tobytes() == rows.tobytes()
        st, mem = _mem(g)
        assert st["capacity"] >= 730 and mem == st["capacity"] * d * 1
        g.raw_clear()
        assert g.raw_count() == 0 and g.raw_elem_bytes() == 1 and g.raw_elem_type() == ETYPE[dtype]
        g.raw_append(rows[:10])
        assert g.raw_gets(np.arange(10)).tobytes() == rows[:10].tobytes()
    finally:
        g.close()


@pytest.mark.parametrize("in_place", [True, False], ids=["mapped", "reallocating"])
def test_appends_across_a_capacity_growth(in_place, monkeypatch):
    """rows of d bytes through the store's growth machinery: the mapped range grows by chunks of 64 MB (524288 rows of
    d = 128; their fp32 goes up in pieces of 64 MB), the reallocating store (GAMMA_HIP_NO_RAW_VMM) from 1024 rows; the second
    append crosses the capacity.  Accounting: capacity x d x 1 bytes."""
    d = 128
    if not in_place:
        monkeypatch.setenv("GAMMA_HIP_NO_RAW_VMM", "1")
    n0 = 524000 if in_place else 1000
    rows = np.random.default_rng(11).integers(0, 256, size=(n0 + 300 + 100, d), dtype=np.uint8).astype(np.float32)
    g = api.GammaHip(0)
    try:
        g.raw_init(d, "uint8")
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
        assert g.total_mem_bytes() == st["capacity"] * d * 1
        sel = np.concatenate([np.arange(0, n0, 997), np.arange(n0 - 5, len(rows))])
        assert g.raw_gets(sel).tobytes() == rows[sel].tobytes()
    finally:
        g.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_refused_value_changes_nothing(dtype):
    lo, hi = RANGE[dtype]
    g = api.GammaHip(0)
    try:
        d = 20
        g.raw_init(d, dtype)
        rows = ints(50, d, dtype, 1)
        g.raw_append(rows)
        before = _mem(g)
        p = lambda a: a.ctypes.data_as(_lib.f32p)
        vids = np.arange(10, 40, dtype=np.int64)
        for bad in (0.5, np.nan, np.inf, -np.inf, hi + 1.0, lo - 1.0, 1e-3, 3e38):
            x = ints(30, d, dtype, 2)
            x[17, 3] = bad                      # in the middle of the batch
            calls = [lambda: g.L.gamma_hip_raw_append(g.h, 30, p(x)),
                     lambda: g.L.gamma_hip_raw_write(g.h, 40, 30, p(x)),
                     lambda: g.L.gamma_hip_raw_update(g.h, 7, p(x[17])),
                     lambda: g.L.gamma_hip_raw_update_batch(g.h, 30, vids.ctypes.data_as(_lib.i64p), p(x))]
            for i, call in enumerate(calls):
                assert call() == EINVAL
                msg = g.L.gamma_hip_last_error(g.h)
                assert dtype.encode() in msg and (b"position 3 " if i == 2 else b"position 343 ") in msg, msg
                assert _mem(g) == before and g.raw_count() == 50
                assert g.raw_gets(np.arange(50)).tobytes() == rows.tobytes()
    finally:
        g.close()


# ---- search parity against the oracle over the fp32 base, and against an fp32 store ---------------------------------
# d 8: no tail; 12: the 4-lane tail; 15: the masked tail (and byte loads); 24: d % 16 != 0 with d % 4 == 0; 100: dword loads with
# a 4-lane tail; 128: the 128-element unroll; 136: one unroll span and dword loads; 272: two unroll spans and one more chunk
SHAPES = [(8, 4), (12, 4), (15, 5), (24, 8), (100, 4), (128, 16), (136, 8), (272, 16)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("metric", [api.METRIC_L2, api.METRIC_IP], ids=["l2", "ip"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "d%d_m%d" % s)
def test_search_parity(shape, metric, dtype):
    d, M = shape
    c = _case(d, M, metric, dtype)
    g, g32 = _handle(c), _handle(c, dtype="float32")
    try:
        assert g.raw_elem_bytes() == 1 and g32.raw_elem_bytes() == 4 and g32.raw_elem_type() == 0
        for nq in (1, 8, 300):                 # 1: the regular chain of a single-query call with has_rank
            for R in (32, 100, 200):
                _check(g, c["oracle"], c["q"][:nq], 10, 8, R, metric, g32=g32)
        assert g.ties_not_honoured() == 0
    finally:
        g.close()
        g32.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(8, 4), (15, 5), (128, 16)], ids=lambda s: "d%d_m%d" % s)
def test_byte_valued_queries_tie_and_are_replayed(shape, dtype):
    """byte-valued queries over byte-valued rows: every exact distance is a small integer, and half of the rows are twins of
    the other half, so equal neighbouring distances are everywhere; their order is the reference heaps' (inline replay, and
    the deferred replay on the side stream through the _wait entry)"""
    import torch
    d, M = shape
    a = ints(N // 2, d, dtype, 500 + d)
    base = np.ascontiguousarray(np.concatenate([a, a])[np.random.default_rng(9).permutation(N)])
    for metric in (api.METRIC_L2, api.METRIC_IP):
        c = _case(d, M, metric, dtype, base=base, tag="twins")
        o = c["oracle"]
        q, k, P, R = c["qb"], 10, 8, 100
        g, g32 = _handle(c), _handle(c, dtype="float32")
        try:
            for nq in (300, 8, 1):
                g.tie_stats(reset=True)
                D, _ = _check(g, o, q[:nq], k, P, R, metric, g32=g32)
                assert (D[:, 1:] == D[:, :-1]).any()
                assert nq == 1 or g.tie_stats()["replayed"] > 0
            D, I = o.search(q, k, P, recall_num=R, has_rank=True, metric=metric, ctx=B.make_ctx(**WIDE))
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
            g32.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_recall_num_beyond_the_fused_kernel(dtype):
    """recall_num 1100: launch_rerank_dist over byte rows, the selection, the tie flags made afterwards"""
    for d, M in ((128, 16), (15, 5), (100, 4)):
        c = _case(d, M, api.METRIC_L2, dtype)
        g, g32 = _handle(c), _handle(c, dtype="float32")
        try:
            _check(g, c["oracle"], c["q"][:40], 10, 8, 1100, c["metric"], g32=g32)
        finally:
            g.close()
            g32.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_unfused_path_without_exact_ties(dtype):
    """nq = 100 with exact ties off for the request: k_rerank_dist + selection (Gaussian queries: no ties to honour)"""
    for d, M, metric in ((136, 8, api.METRIC_IP), (24, 8, api.METRIC_L2), (15, 5, api.METRIC_IP), (272, 16, api.METRIC_L2)):
        c = _case(d, M, metric, dtype)
        g, g32 = _handle(c), _handle(c, dtype="float32")
        try:
            _check(g, c["oracle"], c["q"][:100], 10, 8, 200, metric, exact_ties=-1, g32=g32)
            _check(g, c["oracle"], c["q"][:300], 10, 8, 200, metric, exact_ties=-1, g32=g32)
        finally:
            g.close()
            g32.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_without_rank(dtype):
    """has_rank off: the store is not read; a single-query call takes the small-batch chain"""
    c = _case(100, 4, api.METRIC_L2, dtype)
    g, g32 = _handle(c), _handle(c, dtype="float32")
    try:
        for nq in (1, 8, 300):
            _check(g, c["oracle"], c["q"][:nq], 10, 8, 200, c["metric"], has_rank=False, g32=g32)
    finally:
        g.close()
        g32.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_score_window(dtype):
    for d, M, metric in ((128, 16, api.METRIC_L2), (12, 4, api.METRIC_IP)):
        c = _case(d, M, metric, dtype)
        g, g32 = _handle(c), _handle(c, dtype="float32")
        try:
            q = c["q"][:300]
            D, _ = _check(g, c["oracle"], q, 10, 8, 200, metric)
            lo, hi = sorted((float(np.median(D[:, 2])), float(np.median(D[:, 7]))))
            _check(g, c["oracle"], q, 10, 8, 200, metric, lo=lo, hi=hi, g32=g32)
            _check(g, c["oracle"], q[:8], 10, 8, 200, metric, lo=lo, hi=hi, g32=g32)
        finally:
            g.close()
            g32.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_deleted_docs_and_range_filter(dtype):
    c = _case(136, 8, api.METRIC_L2, dtype)
    rng = np.random.default_rng(3)
    dead = rng.choice(N, N // 10, replace=False)
    bm = np.zeros(N // 8 + 1, np.uint8)
    np.bitwise_or.at(bm, dead >> 3, (1 << (dead & 7)).astype(np.uint8))
    allowed = np.nonzero(rng.random(N) < 0.6)[0]
    g, g32 = _handle(c), _handle(c, dtype="float32")
    try:
        g.bitmap_upload(bm, N)
        g32.bitmap_upload(bm, N)
        for nq in (8, 300):
            _check(g, c["oracle"], c["q"][:nq], 10, 8, 200, c["metric"],
                   ctx_kw=dict(docids_bitmap=bm, range_filters=[B.make_range_filter(allowed)]),
                   arg_kw=dict(range_filters=[api.make_range_filter(allowed)]), g32=g32)
    finally:
        g.close()
        g32.close()


# ---- other handles ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_four_bit_handle(dtype):
    d, nlist, M = 32, 16, 8
    base = ints(N, d, dtype, 41)
    cc, pq = PR.train(base[:3000], nlist, M)
    B.lib().go_set_assign_mode(-1)
    lno, codes = PR.encode(base, cc, pq)
    ix = PR.Index(cc, pq, PR.build_lists(lno, codes, nlist), raw=base)
    g, g32 = api.GammaHip(0), api.GammaHip(0)
    try:
        for h, t in ((g, dtype), (g32, "float32")):
            h.ivfpq4_init(d, nlist, M, api.METRIC_L2)
            h.ivfpq_set_trained(cc, pq, None)
            h.raw_init(d, t)
            h.raw_append(base)
            h.add(base, 0)
        q = gauss(300, d, dtype, 42)
        for nq in (8, 300):
            args = api.SearchArgs(metric=api.METRIC_L2, nprobe=8, recall_num=100, has_rank=True, **WIDE)
            Dg, Ig = g.ivfpq_search(q[:nq], 10, args)
            sg = g.last_stages(nq, 8, 100)
            D, I, st = ix.search(q[:nq], 10, 8, recall_num=100, has_rank=True, l2=True, min_score=-3e38, max_score=3e38)
            compare_search_exact(D, I, st, Dg, Ig, sg)
            Df, If = g32.ivfpq_search(q[:nq], 10, args)
            assert Dg.tobytes() == Df.tobytes() and Ig.tobytes() == If.tobytes()
    finally:
        g.close()
        g32.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_handle_with_an_opq_matrix(dtype):
    d, nlist, M, metric = 32, 16, 8, api.METRIC_L2
    A = OR.random_rotation(d, 100 + d)
    base = ints(N, d, dtype, 51)

    g, g32 = api.GammaHip(0), api.GammaHip(0)
    try:
        for h in (g, g32):
            h.ivfpq_init(d, nlist, M, 8, metric)
            h.opq_set(A)
        base_rot = g.opq_apply(base)
        o, cc, pq = OR.build_oracle(base_rot, nlist, M, metric)
        for h, t in ((g, dtype), (g32, "float32")):
            h.ivfpq_set_trained(cc, pq, None)
            h.raw_init(d, t)
            h.raw_append(base)
            h.add(base, 0)
        for nq, R in ((8, 50), (300, 50)):
            q = OR.pick_queries(o, base, A, gauss(nq + 40, d, dtype, 52), nq, 10, 8, R, metric)
            q_rot = g.opq_apply(q)
            D, I, st = OR.search_ref(o, base, q, q_rot, 10, 8, R, True, metric, min_score=-3e38, max_score=3e38)
            args = api.SearchArgs(metric=metric, nprobe=8, recall_num=R, has_rank=True, **WIDE)
            Dg, Ig = g.ivfpq_search(q, 10, args)
            compare_search_exact(D, I, st, Dg, Ig, g.last_stages(nq, 8, R))
            Df, If = g32.ivfpq_search(q, 10, args)
            assert Dg.tobytes() == Df.tobytes() and Ig.tobytes() == If.tobytes()
    finally:
        g.close()
        g32.close()


# ---- realtime -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_update_batch_rewrites_the_rows(dtype):
    c = _case(24, 8, api.METRIC_L2, dtype)
    o = _new_oracle(c)                     # this test changes its oracle
    raw = c["base"].copy()
    g, g32 = _handle(c, o=o), _handle(c, dtype="float32", o=o)
    try:
        rng = np.random.default_rng(12)
        vids = rng.choice(N, 50, replace=False).astype(np.int64)
        vecs = ints(50, c["d"], dtype, 77)
        for h in (g, g32):
            h.update_batch(vids, vecs)
            h.raw_update_batch(vids, vecs)
        B.lib().go_set_assign_mode(-1)
        try:
            for v, x in zip(vids, vecs):
                o.update(int(v), x)
        finally:
            B.lib().go_set_assign_mode(0)
        raw[vids] = vecs
        o.set_raw(raw)
        for l in range(c["nlist"]):
            ids, cds = g.get_list(l)
            oi, oc = o.get_list(l)
            assert np.array_equal(ids, oi) and cds.tobytes() == oc.tobytes(), "list %d after Update" % l
        for nq in (8, 300):
            _check(g, o, c["q"][:nq], 10, 8, 200, c["metric"], g32=g32)
        # an Add behind it: rows and keys of new vectors
        extra = ints(64, c["d"], dtype, 78)
        for h in (g, g32):
            h.raw_append(extra)
            h.add(extra, N)
        B.lib().go_set_assign_mode(1)
        try:
            assert o.add(extra)
        finally:
            B.lib().go_set_assign_mode(0)
        o.set_raw(np.concatenate([raw, extra]))
        _check(g, o, c["q"][:300], 10, 8, 200, c["metric"], g32=g32)
    finally:
        g.close()
        g32.close()


# ---- refusals -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_readers_of_fp32_rows_refuse_the_byte_store(dtype):
    import torch
    c = _case(24, 8, api.METRIC_L2, dtype)
    g = _handle(c)
    L = g.L

    def refused(rc):
        msg = L.gamma_hip_last_error(g.h)
        assert rc == EUNSUPPORTED and b"8-bit" in msg and b"gamma_hip_raw_init_i8" in msg, (rc, msg)

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
        tex = torch.full((8, 50), 1.0, dtype=torch.float32, device="cuda")
        toff = torch.zeros((8, 64), dtype=torch.int32, device="cuda")
        tD = torch.empty((8, 10), dtype=torch.float32, device="cuda")
        tI = torch.empty((8, 10), dtype=torch.int64, device="cuda")
        refused(L.gamma_hip_ivfpq_shard_exact(g.h, args.ref(), 8, tq.data_ptr(), tids.data_ptr(), 50, tex.data_ptr()))
        refused(L.gamma_hip_ivfpq_shard_export_exact(g.h, args.ref(), 8, tq.data_ptr(), tex.data_ptr(), tids.data_ptr(),
                                                     toff.data_ptr(), 50, tex.data_ptr(), tex.data_ptr()))
        # merges with has_rank and no travelled distances: this handle would have to read its rows
        refused(L.gamma_hip_ivfpq_merge_rerank(g.h, args.ref(), 1, 8, tq.data_ptr(), 10, tex.data_ptr(), tids.data_ptr(), 0, 8,
                                               tD.data_ptr(), tI.data_ptr()))
        refused(L.gamma_hip_ivfpq_merge_replay(g.h, C.addressof(args.p), 1, 8, tq.data_ptr(), 50, tex.data_ptr(),
                                               tids.data_ptr(), toff.data_ptr(), 10, toff.data_ptr(), tD.data_ptr(),
                                               tI.data_ptr()))
    finally:
        g.close()
    g = api.GammaHip(0)
    try:
        g.ivfflat_init(c["d"], c["nlist"], c["metric"])
        g.ivfflat_set_trained(c["cc"])
        g.raw_init(c["d"], dtype)
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
        g.raw_init(8, "uint8")
        assert g.L.gamma_hip_raw_init(g.h, 8) == EINVAL
        assert g.L.gamma_hip_raw_init_f16(g.h, 8) == EINVAL
        assert g.L.gamma_hip_raw_init_i8(g.h, 8, 1) == EINVAL       # the other byte type
        assert g.L.gamma_hip_raw_init_i8(g.h, 12, 0) == EINVAL      # another d
        assert g.L.gamma_hip_raw_init_i8(g.h, 8, 0) == 0
        assert g.raw_elem_type() == 2
        with pytest.raises(ValueError):
            g.raw_init(8, "bfloat16")
    finally:
        g.close()
    g = api.GammaHip(0)
    try:
        g.raw_init(8, "float16")
        assert g.L.gamma_hip_raw_init_i8(g.h, 8, 0) == EINVAL and g.raw_elem_type() == 1
    finally:
        g.close()
