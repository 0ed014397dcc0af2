"""GPU: the scalar-quantised raw store (gamma_hip_raw_init_sq8) through api.GammaHip.

The store is lossy, and nothing else is: the rows it holds are W = decode(encode(base)) by the arithmetic of include/gamma_hip.h,
which tests/sq8_ref.py restates in numpy bit for bit.  The complete expected result of a search is therefore the CPU oracle that
was added the fp32 base (training, lists and codes see the caller's rows) and handed W as its raw rows, and a handle with an sq8
store answers byte for byte what a handle with an fp32 store that was appended W answers.  Searches are compared strictly --
labels and distance bits at every rank, coarse and recall stage included, no query and no rank excluded.

The base: Gaussian rows with a scale and an offset of their own per dimension, every third dimension negative throughout, one
dimension constant; the ranges are trained on the first 3000 rows and the other 3000 are drawn wider, so values clip at both
ends."""
import ctypes as C

import numpy as np
import pytest

from gamma_amd import _lib, api
from oracle import binding as B
from tests import opq_ref as OR
from tests import pq4_ref as PR
from tests import sq8_ref as S
from tests.parity import compare_exact, compare_search_exact

pytestmark = pytest.mark.gpu

N = 6000
WIDE = dict(min_score=-3e38, max_score=3e38)
EINVAL, EUNSUPPORTED = -1, -6   # include/gamma_hip.h
_trained, _cases = {}, {}


def make_base(d, seed, n=N):
    return np.concatenate([S.rows(n // 2, d, seed), S.rows(n - n // 2, d, seed + 1, wide=1.6)])


def trained_store(d, train):
    """a handle with an empty sq8 store whose ranges were trained on the device, and the ranges (checked against numpy)"""
    g = api.GammaHip(0)
    g.raw_init(d, "sq8")
    g.raw_sq8_train(train)
    vmin, vmax = g.raw_sq8_get_ranges()
    assert np.array_equal(vmin, train.min(axis=0)) and np.array_equal(vmax, train.max(axis=0))
    return g, vmin, vmax


def _new_oracle(c):
    o = B.OracleIVFPQ(c["d"], c["nlist"], c["M"], 8, c["metric"])
    o.set_trained(c["cc"], c["pq"], None)
    B.lib().go_set_assign_mode(0)
    assert o.add(c["base"])
    o.set_raw(c["W"])
    return o


def _case(d, M, metric, nlist=16, base=None, tag=""):
    """base, its ranges (numpy's minimum / maximum of the first half) and stored rows W, queries, the trained state (once per
    shape) and the oracle that lists the fp32 base and re-ranks over W (once per shape and metric; left unchanged)"""
    tkey = (d, M, nlist, tag)
    if tkey not in _trained:
        if base is None:
            base = make_base(d, 100 + d)
        vmin, vmax = base[:N // 2].min(axis=0), base[:N // 2].max(axis=0)
        W = S.stored(base, vmin, vmax)
        if not tag:
            step, inv = S.params(vmin, vmax)
            codes = S.encode(base[N // 2:], vmin, inv)
            assert (codes == 0).any() and (codes == 255).any() and (base[N // 2:] < vmin).any() and (base[N // 2:] > vmax).any()
            assert d == 1 or (step == 0).sum() == 1               # the constant dimension
        cc, pq = B.ivfpq_train(base[:3000], nlist, M)
        _trained[tkey] = dict(d=d, M=M, nlist=nlist, base=base, W=W, vmin=vmin, vmax=vmax, q=S.rows(300, d, 7 + d), cc=cc, pq=pq)
    key = tkey + (metric,)
    if key not in _cases:
        c = dict(_trained[tkey], metric=metric)
        c["oracle"] = _new_oracle(c)
        _cases[key] = c
    return _cases[key]


def _handle(c, dtype="sq8", o=None):
    """a handle holding exactly the oracle's lists; an sq8 store trained on the first half of the base and appended the fp32
    base, or an fp32 store appended W"""
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
    if dtype == "sq8":
        g.raw_sq8_train(c["base"][:N // 2])
        vmin, vmax = g.raw_sq8_get_ranges()
        assert np.array_equal(vmin, c["vmin"]) and np.array_equal(vmax, c["vmax"])
        g.raw_append(c["base"])
    else:
        g.raw_append(c["W"])
    return g


def _check(g, o, q, k, P, R, metric, has_rank=True, exact_ties=0, ctx_kw=None, arg_kw=None, lo=-3e38, hi=3e38, g32=None):
    """the handle against the oracle; with g32 (a handle with an fp32 store of W and the same lists) also byte for byte against it"""
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
    return g.raw_stats(), g.total_mem_bytes()


TABLE = 16   # bytes per dimension: the decode table {step, vmin} and the encode table {inv, vmin}


# ---- conversion and writers ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 15, 20, 128])
def test_conversion_and_writers(d):
    rows = make_base(d, d, n=700)
    g = api.GammaHip(0)
    try:
        assert g.raw_elem_type() == 0
        g.close()
        g, vmin, vmax = trained_store(d, rows[:350])
        assert g.raw_elem_bytes() == 1 and g.raw_elem_type() == 4
        rows.reshape(-1)[300] = -0.0
        W = S.stored(rows, vmin, vmax)
        g.raw_append(rows[:100])
        g.raw_append(rows[100:101])
        g.raw_append(rows[101:700])
        assert g.raw_count() == 700
        assert g.raw_gets(np.arange(700)).tobytes() == W.tobytes()
        # raw_write (overlapping, idempotent, may extend), raw_update, raw_update_batch (a vid named twice: the last wins; one
        # beyond the store and a negative one: skipped)
        more = S.rows(40, d, d + 1, wide=2.0)
        g.raw_write(690, more)
        g.raw_write(690, more)
        W = np.concatenate([W[:690], S.stored(more, vmin, vmax)])
        assert g.raw_count() == 730
        one = S.rows(1, d, d + 3, wide=3.0)[0]
        g.raw_update(5, one)
        W[5] = S.stored(one[None, :], vmin, vmax)[0]
        uv = np.array([3, 729, 17, 3, 100000, -1], dtype=np.int64)
        ux = S.rows(6, d, d + 2, wide=1.5)
        g.raw_update_batch(uv, ux)
        uw = S.stored(ux, vmin, vmax)
        W[729], W[17], W[3] = uw[1], uw[2], uw[3]
        assert g.raw_gets(np.arange(730)).tobytes() == W.tobytes()
        st, mem = _mem(g)
        assert st["capacity"] >= 730 and mem == st["capacity"] * d * 1 + TABLE * d
        # raw_clear keeps type and ranges
        g.raw_clear()
        assert g.raw_count() == 0 and g.raw_elem_bytes() == 1 and g.raw_elem_type() == 4
        v2, x2 = g.raw_sq8_get_ranges()
        assert v2.tobytes() == vmin.tobytes() and x2.tobytes() == vmax.tobytes()
        g.raw_append(rows[:10])
        assert g.raw_gets(np.arange(10)).tobytes() == S.stored(rows[:10], vmin, vmax).tobytes()
    finally:
        g.close()


@pytest.mark.parametrize("in_place", [True, False], ids=["mapped", "reallocating"])
def test_appends_across_a_capacity_growth(in_place, monkeypatch):
    """rows of d bytes through the byte store's growth machinery: the mapped range grows by chunks of 64 MB (524288 rows of
    d = 128; their fp32 goes up in pieces of 64 MB), the reallocating store (GAMMA_HIP_NO_RAW_VMM) from 1024 rows; the second
    append crosses the capacity.  Accounting: capacity x d x 1 bytes plus the tables; a quarter of an fp32 store of the same
    capacity."""
    d = 128
    if not in_place:
        monkeypatch.setenv("GAMMA_HIP_NO_RAW_VMM", "1")
    n0 = 524000 if in_place else 1000
    block = make_base(d, 11, n=4096)
    rows = np.ascontiguousarray(np.resize(block, (n0 + 300 + 100, d)))
    g, vmin, vmax = trained_store(d, block[:2048])
    try:
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
        assert g.total_mem_bytes() == st["capacity"] * d * 1 + TABLE * d
        assert 4 * (g.total_mem_bytes() - TABLE * d) == st["capacity"] * d * 4      # a quarter of fp32 rows of that capacity
        sel = np.concatenate([np.arange(0, n0, 997), np.arange(n0 - 5, len(rows))])
        assert g.raw_gets(sel).tobytes() == S.stored(rows[sel], vmin, vmax).tobytes()
    finally:
        g.close()


def test_a_refused_value_changes_nothing():
    d = 20
    rows = make_base(d, 1, n=100)
    g, vmin, vmax = trained_store(d, rows[:50])
    try:
        g.raw_append(rows[:50])
        before = _mem(g)
        W = S.stored(rows[:50], vmin, vmax)
        p = lambda a: a.ctypes.data_as(_lib.f32p)
        vids = np.arange(10, 40, dtype=np.int64)
        for bad in (np.nan, np.inf, -np.inf):
            x = rows[50:80].copy()
            x[17, 3] = bad                      # in the middle of the batch
            calls = [lambda: g.L.gamma_hip_raw_append(g.h, 30, p(x)),
                     lambda: g.L.gamma_hip_raw_write(g.h, 40, 30, p(x)),
                     lambda: g.L.gamma_hip_raw_update(g.h, 7, p(x[17])),
                     lambda: g.L.gamma_hip_raw_update_batch(g.h, 30, vids.ctypes.data_as(_lib.i64p), p(x))]
            for i, call in enumerate(calls):
                assert call() == EINVAL
                msg = g.L.gamma_hip_last_error(g.h)
                assert b"sq8" in msg and (b"position 3 " if i == 2 else b"position 343 ") in msg, msg
                assert _mem(g) == before and g.raw_count() == 50
                assert g.raw_gets(np.arange(50)).tobytes() == W.tobytes()
        # finite values far outside the ranges, and -0.0, are accepted: they clip
        x = rows[50:51].copy()
        x[0, :3] = (3e38, -3e38, -0.0)
        g.raw_append(x)
        assert g.raw_gets(np.array([50])).tobytes() == S.stored(x, vmin, vmax).tobytes()
    finally:
        g.close()


def test_ranges_come_first_and_change_only_while_the_store_is_empty():
    d = 12
    rows = make_base(d, 2, n=100)
    p = lambda a: a.ctypes.data_as(_lib.f32p)
    g = api.GammaHip(0)
    try:
        g.raw_init(d, "sq8")
        L = g.L
        vids = np.arange(3, dtype=np.int64)
        lo, hi = np.empty(d, np.float32), np.empty(d, np.float32)
        assert L.gamma_hip_raw_sq8_get_ranges(g.h, p(lo), p(hi)) == EINVAL
        # writers before any ranges exist
        for call in (lambda: L.gamma_hip_raw_append(g.h, 3, p(rows)), lambda: L.gamma_hip_raw_write(g.h, 0, 3, p(rows))):
            assert call() == EINVAL
            assert b"no ranges" in L.gamma_hip_last_error(g.h)
            assert g.raw_count() == 0 and g.total_mem_bytes() == 0
        assert L.gamma_hip_raw_append(g.h, 0, p(rows)) == 0              # n == 0 is no write
        # refused ranges leave none
        vmin, vmax = rows[:50].min(axis=0), rows[:50].max(axis=0)
        for j, (a, b) in enumerate([(np.nan, 1.0), (0.0, np.inf), (2.0, 1.0), (-3e38, 3e38)]):
            bmin, bmax = vmin.copy(), vmax.copy()
            bmin[j], bmax[j] = a, b
            assert L.gamma_hip_raw_sq8_set_ranges(g.h, p(bmin), p(bmax)) == EINVAL
            assert L.gamma_hip_raw_sq8_get_ranges(g.h, p(lo), p(hi)) == EINVAL
        bad = rows[:50].copy()
        bad[7, 2] = np.nan
        assert L.gamma_hip_raw_sq8_train(g.h, 50, p(bad)) == EINVAL and L.gamma_hip_raw_sq8_train(g.h, 0, p(bad)) == EINVAL
        g.raw_sq8_set_ranges(vmin, vmax)
        g.raw_append(rows[:60])
        assert g.raw_gets(np.arange(60)).tobytes() == S.stored(rows[:60], vmin, vmax).tobytes()
        # a non-empty store keeps its ranges
        assert L.gamma_hip_raw_sq8_set_ranges(g.h, p(vmin), p(vmax)) == EINVAL
        assert b"holds rows" in L.gamma_hip_last_error(g.h)
        assert L.gamma_hip_raw_sq8_train(g.h, 50, p(rows)) == EINVAL
        a, b = g.raw_sq8_get_ranges()
        assert a.tobytes() == vmin.tobytes() and b.tobytes() == vmax.tobytes()
        # ... until raw_clear, which keeps them; then they may change
        g.raw_clear()
        a, b = g.raw_sq8_get_ranges()
        assert a.tobytes() == vmin.tobytes() and b.tobytes() == vmax.tobytes()
        wmin, wmax = rows.min(axis=0), rows.max(axis=0) + np.float32(1.0)
        g.raw_sq8_set_ranges(wmin, wmax)
        g.raw_append(rows)
        assert g.raw_gets(np.arange(100)).tobytes() == S.stored(rows, wmin, wmax).tobytes()
    finally:
        g.close()
    # the ranges calls on a store of another type
    g = api.GammaHip(0)
    try:
        g.raw_init(d, "uint8")
        assert g.L.gamma_hip_raw_sq8_set_ranges(g.h, p(vmin), p(vmax)) == EINVAL
        assert g.L.gamma_hip_raw_sq8_train(g.h, 50, p(rows)) == EINVAL
    finally:
        g.close()


def test_training_in_several_pieces_and_with_both_zeros():
    """a training set larger than one staging piece (64 MB of fp32: 16384 rows of d = 1024 and a few more), and a dimension
    whose minimum is a zero of either sign: the answer is +0.0"""
    d = 1024
    block = make_base(d, 21, n=512)
    block[:, 9] = np.abs(block[:, 9])
    block[3, 9], block[200, 9] = -0.0, 0.0
    x = np.ascontiguousarray(np.resize(block, (16384 + 77, d)))
    x[16384 + 50, 4] = 1e6                   # the maximum sits in the second piece
    x[5, 6] = -1e6                           # the minimum in the first
    g = api.GammaHip(0)
    try:
        g.raw_init(d, "sq8")
        g.raw_sq8_train(x)
        vmin, vmax = g.raw_sq8_get_ranges()
        assert np.array_equal(vmin, x.min(axis=0)) and np.array_equal(vmax, x.max(axis=0))
        assert vmax[4] == 1e6 and vmin[6] == -1e6 and vmin[9] == 0 and not np.signbit(vmin[9])
    finally:
        g.close()


# ---- search parity against the oracle over W, and against an fp32 store of W -----------------------------------------
# d 8: no tail; 12: the 4-lane tail; 15: the masked tail (and byte loads); 24: d % 16 != 0 with d % 4 == 0; 100: dword loads with
# a 4-lane tail; 128: the 128-element unroll; 136: one unroll span and dword loads; 272: two unroll spans and one more chunk
SHAPES = [(8, 4), (12, 4), (15, 5), (24, 8), (100, 4), (128, 16), (136, 8), (272, 16)]


@pytest.mark.parametrize("metric", [api.METRIC_L2, api.METRIC_IP], ids=["l2", "ip"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "d%d_m%d" % s)
def test_search_parity(shape, metric):
    d, M = shape
    c = _case(d, M, metric)
    g, g32 = _handle(c), _handle(c, dtype="float32")
    try:
        assert g.raw_elem_bytes() == 1 and g.raw_elem_type() == 4 and g32.raw_elem_bytes() == 4 and g32.raw_elem_type() == 0
        assert g.raw_gets(np.arange(N)).tobytes() == c["W"].tobytes()
        # store bytes: a quarter of the fp32 store's up to capacity rounding (both stores round to whole 64 MB chunks or, reallocating,
        # to the same number of rows), plus the tables
        s8, s32 = g.raw_stats(), g32.raw_stats()
        assert g.total_mem_bytes() - g32.total_mem_bytes() == s8["capacity"] * d + TABLE * d - s32["capacity"] * d * 4
        for nq in (1, 8, 300):                 # 1: the regular chain of a single-query call with has_rank
            for R in (32, 100, 200):
                _check(g, c["oracle"], c["q"][:nq], 10, 8, R, metric, g32=g32)
        assert g.ties_not_honoured() == 0
    finally:
        g.close()
        g32.close()


@pytest.mark.parametrize("shape", [(8, 4), (15, 5), (128, 16)], ids=lambda s: "d%d_m%d" % s)
def test_twin_rows_tie_and_are_replayed(shape):
    """every row appears twice: the twins' decoded rows are identical, so equal neighbouring exact distances are everywhere; their
    order is the reference heaps' (inline replay, and the deferred replay on the side stream through the _wait entry)"""
    import torch
    d, M = shape
    a = make_base(d, 500 + d, n=N // 2)
    base = np.ascontiguousarray(np.concatenate([a, a])[np.random.default_rng(9).permutation(N)])
    for metric in (api.METRIC_L2, api.METRIC_IP):
        c = _case(d, M, metric, base=base, tag="twins")
        o = c["oracle"]
        q, k, P, R = c["q"], 10, 8, 100
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


def test_recall_num_beyond_the_fused_kernel():
    """recall_num 1100: launch_rerank_dist over sq8 rows, the selection, the tie flags made afterwards"""
    for d, M in ((128, 16), (15, 5), (100, 4)):
        c = _case(d, M, api.METRIC_L2)
        g, g32 = _handle(c), _handle(c, dtype="float32")
        try:
            _check(g, c["oracle"], c["q"][:40], 10, 8, 1100, c["metric"], g32=g32)
        finally:
            g.close()
            g32.close()


def test_unfused_path_without_exact_ties():
    """nq = 100 with exact ties off for the request: k_rerank_dist + selection (real-valued rows: no ties to honour)"""
    for d, M, metric in ((136, 8, api.METRIC_IP), (24, 8, api.METRIC_L2), (15, 5, api.METRIC_IP), (272, 16, api.METRIC_L2)):
        c = _case(d, M, metric)
        g, g32 = _handle(c), _handle(c, dtype="float32")
        try:
            _check(g, c["oracle"], c["q"][:100], 10, 8, 200, metric, exact_ties=-1, g32=g32)
            _check(g, c["oracle"], c["q"][:300], 10, 8, 200, metric, exact_ties=-1, g32=g32)
        finally:
            g.close()
            g32.close()


def test_without_rank():
    """has_rank off: the store is not read; a single-query call takes the small-batch chain"""
    c = _case(100, 4, api.METRIC_L2)
    g, g32 = _handle(c), _handle(c, dtype="float32")
    try:
        for nq in (1, 8, 300):
            _check(g, c["oracle"], c["q"][:nq], 10, 8, 200, c["metric"], has_rank=False, g32=g32)
    finally:
        g.close()
        g32.close()


def test_score_window():
    for d, M, metric in ((128, 16, api.METRIC_L2), (12, 4, api.METRIC_IP)):
        c = _case(d, M, metric)
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


def test_deleted_docs_and_range_filter():
    c = _case(136, 8, api.METRIC_L2)
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
def test_four_bit_handle():
    d, nlist, M = 32, 16, 8
    base = make_base(d, 41)
    vmin, vmax = base[:3000].min(axis=0), base[:3000].max(axis=0)
    W = S.stored(base, vmin, vmax)
    cc, pq = PR.train(base[:3000], nlist, M)
    B.lib().go_set_assign_mode(-1)
    lno, codes = PR.encode(base, cc, pq)
    ix = PR.Index(cc, pq, PR.build_lists(lno, codes, nlist), raw=W)
    g, g32 = api.GammaHip(0), api.GammaHip(0)
    try:
        for h, t in ((g, "sq8"), (g32, "float32")):
            h.ivfpq4_init(d, nlist, M, api.METRIC_L2)
            h.ivfpq_set_trained(cc, pq, None)
            h.raw_init(d, t)
            if t == "sq8":
                h.raw_sq8_train(base[:3000])
            h.raw_append(base if t == "sq8" else W)
            h.add(base, 0)
        q = S.rows(300, d, 42)
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


def test_handle_with_an_opq_matrix():
    d, nlist, M, metric = 32, 16, 8, api.METRIC_L2
    A = OR.random_rotation(d, 100 + d)
    base = make_base(d, 51)
    vmin, vmax = base[:3000].min(axis=0), base[:3000].max(axis=0)
    W = S.stored(base, vmin, vmax)                 # the store holds the caller's rows, not the rotated ones
    g, g32 = api.GammaHip(0), api.GammaHip(0)
    try:
        for h in (g, g32):
            h.ivfpq_init(d, nlist, M, 8, metric)
            h.opq_set(A)
        base_rot = g.opq_apply(base)
        o, cc, pq = OR.build_oracle(base_rot, nlist, M, metric)
        for h, t in ((g, "sq8"), (g32, "float32")):
            h.ivfpq_set_trained(cc, pq, None)
            h.raw_init(d, t)
            if t == "sq8":
                h.raw_sq8_train(base[:3000])
            h.raw_append(base if t == "sq8" else W)
            h.add(base, 0)
        for nq, R in ((8, 50), (300, 50)):
            q = OR.pick_queries(o, W, A, S.rows(nq + 40, d, 52), nq, 10, 8, R, metric)
            q_rot = g.opq_apply(q)
            D, I, st = OR.search_ref(o, W, q, q_rot, 10, 8, R, True, metric, min_score=-3e38, max_score=3e38)
            args = api.SearchArgs(metric=metric, nprobe=8, recall_num=R, has_rank=True, **WIDE)
            Dg, Ig = g.ivfpq_search(q, 10, args)
            compare_search_exact(D, I, st, Dg, Ig, g.last_stages(nq, 8, R))
            Df, If = g32.ivfpq_search(q, 10, args)
            assert Dg.tobytes() == Df.tobytes() and Ig.tobytes() == If.tobytes()
    finally:
        g.close()
        g32.close()


# ---- realtime -----------------------------------------------------------------------------------------------------
def test_update_batch_rewrites_the_rows():
    c = _case(24, 8, api.METRIC_L2)
    o = _new_oracle(c)                     # this test changes its oracle
    raw = c["W"].copy()
    g, g32 = _handle(c, o=o), _handle(c, dtype="float32", o=o)
    try:
        rng = np.random.default_rng(12)
        vids = rng.choice(N, 50, replace=False).astype(np.int64)
        vecs = S.rows(50, c["d"], 77, wide=1.5)
        wvecs = S.stored(vecs, c["vmin"], c["vmax"])
        for h, rows in ((g, vecs), (g32, wvecs)):
            h.update_batch(vids, vecs)
            h.raw_update_batch(vids, rows)
        B.lib().go_set_assign_mode(-1)
        try:
            for v, x in zip(vids, vecs):
                o.update(int(v), x)
        finally:
            B.lib().go_set_assign_mode(0)
        raw[vids] = wvecs
        o.set_raw(raw)
        for l in range(c["nlist"]):
            ids, cds = g.get_list(l)
            oi, oc = o.get_list(l)
            assert np.array_equal(ids, oi) and cds.tobytes() == oc.tobytes(), "list %d after Update" % l
        for nq in (8, 300):
            _check(g, o, c["q"][:nq], 10, 8, 200, c["metric"], g32=g32)
        # an Add behind it: rows and keys of new vectors
        extra = S.rows(64, c["d"], 78, wide=1.5)
        wextra = S.stored(extra, c["vmin"], c["vmax"])
        for h, rows in ((g, extra), (g32, wextra)):
            h.raw_append(rows)
            h.add(extra, N)
        B.lib().go_set_assign_mode(1)
        try:
            assert o.add(extra)
        finally:
            B.lib().go_set_assign_mode(0)
        o.set_raw(np.concatenate([raw, wextra]))
        _check(g, o, c["q"][:300], 10, 8, 200, c["metric"], g32=g32)
    finally:
        g.close()
        g32.close()


# ---- refusals -----------------------------------------------------------------------------------------------------
def test_readers_of_other_rows_refuse_the_sq8_store():
    import torch
    c = _case(24, 8, api.METRIC_L2)
    g = _handle(c)
    L = g.L

    def refused(rc):
        msg = L.gamma_hip_last_error(g.h)
        assert rc == EUNSUPPORTED and b"sq8" in msg and b"gamma_hip_raw_init_sq8" in msg, (rc, msg)

    try:
        q = c["q"][:8]
        args = api.SearchArgs(metric=c["metric"], nprobe=8, recall_num=50, has_rank=True, **WIDE)
        D = np.empty((8, 10), np.float32)
        I = np.empty((8, 10), np.int64)
        for on in (False, True):               # whatever the narrow-rows switch says
            g.set_flat_narrow_rows(on)
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
        # the store is still served
        _check(g, c["oracle"], q, 10, 8, 50, c["metric"])
    finally:
        g.close()
    g = api.GammaHip(0)
    try:
        g.ivfflat_init(c["d"], c["nlist"], c["metric"])
        g.ivfflat_set_trained(c["cc"])
        g.raw_init(c["d"], "sq8")
        g.raw_sq8_train(c["base"][:500])
        g.raw_append(c["base"][:500])
        g.add_keys_batch([0], [500], np.arange(500), np.zeros((500, 1), np.uint8))
        for on in (False, True):
            g.set_ivfflat_narrow_rows(on)
            refused(L.gamma_hip_ivfflat_search(g.h, args.ref(), 8, q.ctypes.data_as(_lib.f32p), 10, D.ctypes.data_as(_lib.f32p),
                                               I.ctypes.data_as(_lib.i64p)))
    finally:
        g.close()


def test_element_type_is_fixed_at_init():
    g = api.GammaHip(0)
    try:
        assert g.raw_elem_bytes() == 0
        g.raw_init(8, "sq8")
        assert g.L.gamma_hip_raw_init(g.h, 8) == EINVAL
        assert g.L.gamma_hip_raw_init_f16(g.h, 8) == EINVAL
        assert g.L.gamma_hip_raw_init_i8(g.h, 8, 0) == EINVAL and g.L.gamma_hip_raw_init_i8(g.h, 8, 1) == EINVAL
        assert g.L.gamma_hip_raw_init_sq8(g.h, 12) == EINVAL         # another d
        assert g.L.gamma_hip_raw_init_sq8(g.h, 8) == 0
        assert g.raw_elem_type() == 4 and g.raw_elem_bytes() == 1
        with pytest.raises(ValueError):
            g.raw_init(8, "sq4")
    finally:
        g.close()
    for other, et in (("float32", 0), ("float16", 1), ("uint8", 2), ("int8", 3)):
        g = api.GammaHip(0)
        try:
            g.raw_init(8, other)
            assert g.L.gamma_hip_raw_init_sq8(g.h, 8) == EINVAL and g.raw_elem_type() == et
        finally:
            g.close()
