"""GPU: 4-bit PQ codes (gamma_hip_ivfpq4_init) through api.GammaHip against the yardstick of tests/pq4_ref.py, strictly:
the precomputed table, the codes of _encode, the lists after _add and the trained state of _train bit-equal; searches
through compare_search_exact (coarse stage, recall stage, final table; exact ties on: no query excluded)."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

from gamma_amd import api
from oracle import binding as B
from tests import fixtures
from tests import gen_golden_pq4 as GG
from tests import pq4_ref as PR
from tests.parity import compare_exact, compare_search_exact

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WIDE = dict(min_score=-3e38, max_score=3e38)
_cases = {}


def _case(d, nlist, M, N=4000, integer=False, seed=3):
    """data + the yardstick's trained state, codes and lists (built once per shape)"""
    key = (d, nlist, M, N, integer, seed)
    if key not in _cases:
        base = PR.clustered(N, d, seed, integer=integer)
        cc, pq = PR.train(base[:min(N, 3000)], nlist, M)
        B.lib().go_set_assign_mode(-1)
        lno, codes = PR.encode(base, cc, pq)
        _cases[key] = dict(d=d, nlist=nlist, M=M, N=N, base=base, cc=cc, pq=pq, lno=lno, codes=codes)
    c = _cases[key]
    lists = PR.build_lists(c["lno"], c["codes"], nlist)
    return c, PR.Index(c["cc"], c["pq"], lists, raw=c["base"].copy())


def _handle(c, metric=api.METRIC_L2, bucket_init_size=1000, add=True):
    g = api.GammaHip(0)
    g.ivfpq4_init(c["d"], c["nlist"], c["M"], metric, bucket_init_size)
    g.ivfpq_set_trained(c["cc"], c["pq"], None)
    g.raw_init(c["d"])
    g.raw_append(c["base"])
    if add:
        g.add(c["base"], 0)
    return g


def _check(g, ix, q, k, P, R, has_rank=True, l2=True, lo=-3e38, hi=3e38, filt=None, **kw):
    args = api.SearchArgs(metric=api.METRIC_L2 if l2 else api.METRIC_IP, nprobe=P, recall_num=R, has_rank=has_rank,
                          min_score=lo, max_score=hi, **kw)
    Dg, Ig = g.ivfpq_search(q, k, args)
    sg = g.last_stages(q.shape[0], P, max(R, k))
    D, I, st = ix.search(q, k, P, recall_num=R, has_rank=has_rank, l2=l2, min_score=lo, max_score=hi, filt=filt)
    compare_search_exact(D, I, st, Dg, Ig, sg)
    return Dg, Ig


SHAPES = [(32, 16, 8), (128, 32, 32), (128, 16, 64), (20, 16, 5), (24, 16, 12), (64, 16, 4)]   # (d, nlist, M); the last: dsub 16


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "d%d_l%d_m%d" % s)
def test_table_codes_lists_and_search(shape):
    d, nlist, M = shape
    c, ix = _case(d, nlist, M)
    g = _handle(c)
    try:
        assert g.code_size() == PR.code_size(M)
        assert g.ivfpq_table().tobytes() == ix.T2.tobytes(), "precomputed table"
        lno, codes = g.encode(c["base"][:300])
        assert np.array_equal(lno, c["lno"][:300]) and codes.tobytes() == c["codes"][:300].tobytes(), "encode"
        lno1, codes1 = g.encode(c["base"][:7])   # fewer than 20 vectors: the exact assignment
        rl, rc = PR.encode(c["base"][:7], c["cc"], c["pq"])
        assert np.array_equal(lno1, rl) and codes1.tobytes() == rc.tobytes(), "encode (exact form)"
        for l in range(nlist):
            ids, cds = g.get_list(l)
            assert np.array_equal(ids, ix.lists[l][0]) and cds.tobytes() == ix.lists[l][1].tobytes(), "list %d" % l
        q = PR.clustered(64, d, 99)
        for l2 in (True, False):          # the index is L2: the second is a per-request metric other than the index's
            for has_rank in (True, False):
                _check(g, ix, q, 10, min(6, nlist), 50, has_rank=has_rank, l2=l2)
        assert g.ties_not_honoured() == 0
    finally:
        g.close()


@pytest.mark.parametrize("nq", [1, 3, 64, 4096])
def test_batch_sizes(nq):
    c, ix = _case(32, 16, 8)
    g = _handle(c)
    try:
        q = PR.clustered(nq, 32, 1000 + nq)
        _check(g, ix, q, 10, 5, 40)
        _check(g, ix, q, 10, 5, 40, has_rank=False)
        assert g.ties_not_honoured() == 0
    finally:
        g.close()


def test_inner_product_index_windows_and_small_recall():
    c, ix = _case(24, 16, 12)
    g = _handle(c, metric=api.METRIC_IP)
    try:
        q = PR.clustered(40, 24, 5)
        _check(g, ix, q, 10, 6, 60, l2=False)
        _check(g, ix, q, 10, 6, 60, l2=True)                      # per-request L2 on an inner-product index
        _check(g, ix, q, 10, 6, 4)                                # recall_num < k
        _check(g, ix, q, 10, 6, 4, has_rank=False)
        D, _ = _check(g, ix, q, 10, 6, 60)
        lo, hi = float(np.median(D[:, 2])), float(np.median(D[:, 7]))
        _check(g, ix, q, 10, 6, 60, lo=lo, hi=hi)                 # score window on the exact distances
        _check(g, ix, q, 10, 6, 60, has_rank=False, lo=lo, hi=hi)   # ... and on the ADC distances
        assert g.ties_not_honoured() == 0
    finally:
        g.close()


def test_deletes_filters_and_vid2docid():
    c, ix = _case(32, 16, 8)
    N = c["N"]
    rng = np.random.default_rng(8)
    g = _handle(c)
    try:
        q = PR.clustered(48, 32, 6)
        deleted = rng.choice(N, N // 5, replace=False)
        g.bitmap_set(deleted)
        g.delete(deleted)
        _check(g, ix, q, 10, 6, 50, filt=PR.Filter(deleted=deleted))
        docs = rng.choice(N, N // 2, replace=False)
        for not_in in (False, True):
            _check(g, ix, q, 10, 6, 50, filt=PR.Filter(deleted=deleted, ranges=[(docs, not_in)]),
                   range_filters=[api.make_range_filter(docs, b_not_in=not_in)])
        # device field filter: an int32 column, [lo, hi] inclusive
        col = rng.integers(0, 100, N).astype(np.int32)
        g.field_append(0, col)
        match = np.nonzero((col >= 20) & (col <= 60))[0]
        _check(g, ix, q, 10, 6, 50, filt=PR.Filter(deleted=deleted, ranges=[(match, False)]),
               field_filters=[(0, 20, 60, True, True)])
        # nq large enough that the call runs over lists compacted under its filter
        qb = PR.clustered(1024, 32, 61)
        _check(g, ix, qb, 10, 6, 50, filt=PR.Filter(deleted=deleted, ranges=[(docs, False)]),
               range_filters=[api.make_range_filter(docs)])
    finally:
        g.close()
    # multi-vector documents: docid = vid2doc[vid]; deletes and ranges are by docid
    g = _handle(c)
    try:
        v2d = (np.arange(N) // 3).astype(np.int32)
        g.vid2docid_append(v2d)
        ddocs = rng.choice(N // 3, N // 12, replace=False)
        g.bitmap_set(ddocs)
        rdocs = rng.choice(N // 3, N // 6, replace=False)
        _check(g, ix, q, 10, 6, 50, filt=PR.Filter(deleted=ddocs, ranges=[(rdocs, True)], vid2doc=v2d),
               range_filters=[api.make_range_filter(rdocs, b_not_in=True)])
    finally:
        g.close()


def test_update_and_compaction_scripts():
    c, ix = _case(32, 16, 8, N=3000)
    N = c["N"]
    rng = np.random.default_rng(12)
    g = _handle(c, bucket_init_size=64)
    try:
        q = PR.clustered(40, 32, 7)
        # Update: new vectors for 150 vids (some stay in their list, most move), in order
        vids = rng.choice(N, 150, replace=False).astype(np.int64)
        vecs = PR.clustered(150, 32, 77)
        g.update_batch(vids, vecs)
        for v, x in zip(vids, vecs):
            g.raw_update(int(v), x)
            ix.update(int(v), x)
            ix.raw[int(v)] = x
        for l in range(c["nlist"]):
            ids, cds = g.get_list(l)
            assert np.array_equal(ids, ix.lists[l][0]) and cds.tobytes() == ix.lists[l][1].tobytes(), "list %d after Update" % l
        _check(g, ix, q, 10, 6, 50)
        # compaction: half of the biggest list deleted (it compacts), a tenth of another (it does not)
        sizes = [int((ix.lists[l][0] >= 0).sum()) for l in range(c["nlist"])]
        order = np.argsort(sizes)
        la, lb = int(order[-1]), int(order[-2])
        live_a = ix.lists[la][0][ix.lists[la][0] >= 0]
        live_b = ix.lists[lb][0][ix.lists[lb][0] >= 0]
        deleted = np.concatenate([live_a[::2], live_b[::10]])
        g.bitmap_set(deleted)
        g.delete(deleted)
        g.compact_if_need()
        for l in range(c["nlist"]):
            lv = ix.lists[l][0]
            ndel = int((lv < 0).sum()) + int(np.isin(lv[lv >= 0], deleted).sum())
            if lv.size and np.float32(ndel) / np.float32(lv.size) >= np.float32(0.3):
                ix.compact(l, deleted)
        assert ix.lists[la][0].size == live_a.size - live_a[::2].size
        for l in range(c["nlist"]):
            ids, cds = g.get_list(l)
            assert np.array_equal(ids, ix.lists[l][0]) and cds.tobytes() == ix.lists[l][1].tobytes(), "list %d after compaction" % l
        _check(g, ix, q, 10, 6, 50, filt=PR.Filter(deleted=deleted))
    finally:
        g.close()


def test_train_on_a_4bit_handle():
    d, nlist, M = 32, 16, 8
    x = PR.clustered(5000, d, 100 + d)   # more than 256 * 16 points: the residual subsample
    gold = np.load(os.path.join(HERE, "golden", "ivfpq4_train.npz"))
    g = api.GammaHip(0)
    try:
        g.ivfpq4_init(d, nlist, M)
        cc, pq = g.ivfpq_train(x, nlist, M)
        assert pq.shape == (M, 16, d // M)
        rc, rp = PR.train(x, nlist, M)
        assert cc.tobytes() == rc.tobytes() and pq.tobytes() == rp.tobytes(), "trained state vs the yardstick"
        assert cc.tobytes() == gold["cc_32_16_8"].tobytes() and pq.tobytes() == gold["pq_32_16_8"].tobytes(), "vs compiled faiss"
    finally:
        g.close()
    g8 = api.GammaHip(0)   # any other handle: 256 centroids per sub-quantizer as before
    try:
        g8.ivfpq_init(d, nlist, M)
        cc8, pq8 = g8.ivfpq_train(x[:3000], nlist, M)
        assert pq8.shape == (M, 256, d // M)
        oc, op = B.ivfpq_train(x[:3000], nlist, M)
        assert cc8.tobytes() == oc.tobytes() and pq8.tobytes() == op.tobytes()
    finally:
        g8.close()


def test_ties_golden():
    """integer-valued data, odd M: equal ADC distances at the recall cut; the recall stage must hold exactly the entries
    compiled faiss kept"""
    z = dict(np.load(os.path.join(HERE, "golden", "ivfpq4_ties_d20.npz")))
    d, nlist, M, P, R = (int(z[k]) for k in ("d", "nlist", "M", "nprobe", "R"))
    lists = GG.lists_of(z)
    g = api.GammaHip(0)
    try:
        g.ivfpq4_init(d, nlist, M)
        g.ivfpq_set_trained(z["cc"], z["pq"], None)
        assert g.ivfpq_table().tobytes() == z["T2"].tobytes()
        g.raw_init(d)
        g.raw_append(z["base"])
        nz = [l for l in range(nlist) if lists[l][0].size]
        g.add_keys_batch(nz, [lists[l][0].size for l in nz], np.concatenate([lists[l][0] for l in nz]),
                         np.concatenate([lists[l][1] for l in nz]))
        ix = PR.Index(z["cc"], z["pq"], lists, raw=z["base"])
        q = z["q"]
        for has_rank in (False, True):
            args = api.SearchArgs(metric=api.METRIC_L2, nprobe=P, recall_num=R, has_rank=has_rank, **WIDE)
            Dg, Ig = g.ivfpq_search(q, 10, args)
            sg = g.last_stages(q.shape[0], P, R)
            D, I, st = ix.search(q, 10, P, recall_num=R, has_rank=has_rank, min_score=-3e38, max_score=3e38)
            gold = dict(coarse_dis=z["coarse_dis"], coarse_idx=z["coarse_idx"], recall_dis=z["recall_dis"], recall_ids=z["recall_ids"])
            compare_search_exact(D, I, gold, Dg, Ig, sg)
        assert g.ties_not_honoured() == 0
    finally:
        g.close()


def test_four_threads_small_host_calls_equal_serial():
    """small host-buffer calls from several threads go through the combining queue: a 4-bit handle is served by it"""
    c, ix = _case(32, 16, 8)
    g = _handle(c)
    try:
        args = api.SearchArgs(metric=api.METRIC_L2, nprobe=6, recall_num=50, has_rank=True, coarse_mode=0, **WIDE)
        qs = [PR.clustered(5, 32, 300 + i) for i in range(24)]
        serial = [g.ivfpq_search(x, 10, args) for x in qs]
        D, I, _ = ix.search(qs[0], 10, 6, recall_num=50, min_score=-3e38, max_score=3e38, coarse_mode=0)
        compare_exact(D, I, serial[0][0], serial[0][1])
        errors = []

        def client(t):
            try:
                for rep in range(10):
                    for i in range(t, len(qs), 4):
                        Dt, It = g.ivfpq_search(qs[i], 10, args)
                        compare_exact(serial[i][0], serial[i][1], Dt, It)
            except BaseException as e:   # noqa: B902 (reported by the main thread)
                errors.append((t, repr(e)))

        th = [threading.Thread(target=client, args=(t,)) for t in range(4)]
        for x in th:
            x.start()
        for x in th:
            x.join()
        assert not errors, errors[:3]
    finally:
        g.close()


def test_device_pointer_calls():
    import torch
    c, ix = _case(32, 16, 8)
    g = _handle(c)
    try:
        dev = torch.device("cuda", 0)
        nq, k = 700, 10
        q = PR.clustered(nq, 32, 41)
        dq = torch.from_numpy(q).to(dev)
        D = torch.empty((nq, k), dtype=torch.float32, device=dev)
        I = torch.empty((nq, k), dtype=torch.int64, device=dev)
        args = api.SearchArgs(metric=api.METRIC_L2, nprobe=6, recall_num=50, has_rank=True, **WIDE)
        Dr, Ir, _ = ix.search(q, k, 6, recall_num=50, min_score=-3e38, max_score=3e38)
        g.ivfpq_search_device(dq.data_ptr(), nq, k, args, D.data_ptr(), I.data_ptr())
        g.synchronize()
        compare_exact(Dr, Ir, D.cpu().numpy(), I.cpu().numpy())
        D.zero_()
        g.ivfpq_search_device_wait(dq.data_ptr(), nq, k, args, D.data_ptr(), I.data_ptr())
        compare_exact(Dr, Ir, D.cpu().numpy(), I.cpu().numpy())
    finally:
        g.close()


def test_unsupported_entries_say_so():
    import torch
    c, _ = _case(32, 16, 8)
    g = _handle(c)
    try:
        dev = torch.device("cuda", 0)
        buf = torch.zeros(1 << 16, dtype=torch.float32, device=dev)
        p = C.c_void_p(buf.data_ptr())
        args = api.SearchArgs(metric=api.METRIC_L2, nprobe=4, recall_num=20, has_rank=False, **WIDE)
        L, h, a = g.L, g.h, args.ref()
        n_out, l_out, mx = C.c_int(0), C.c_void_p(), C.c_int64(0)
        calls = {
            "search_shard": lambda: L.gamma_hip_ivfpq_search_shard(h, a, 4, p, 10, p, p),
            "search_shard_preassigned": lambda: L.gamma_hip_ivfpq_search_shard_preassigned(h, a, 4, p, p, p, 10, p, p),
            "search_shard_bounded": lambda: L.gamma_hip_ivfpq_search_shard_bounded(h, a, 4, p, p, p, 10, p, p, p, None, None),
            "merge_rerank": lambda: L.gamma_hip_ivfpq_merge_rerank(h, a, 1, 4, p, 10, p, p, 0, 4, p, p),
            "merge_rerank_exact": lambda: L.gamma_hip_ivfpq_merge_rerank_exact(h, a, 1, 4, p, 10, p, p, p, 0, 4, p, p),
            "shard_exact": lambda: L.gamma_hip_ivfpq_shard_exact(h, a, 4, p, p, 20, p),
            "shard_cut_flags": lambda: L.gamma_hip_ivfpq_shard_cut_flags(h, 4, p),
            "merge_set_shard_flags": lambda: L.gamma_hip_ivfpq_merge_set_shard_flags(h, p),
            "merge_flagged": lambda: L.gamma_hip_ivfpq_merge_flagged(h, C.byref(n_out), C.byref(l_out)),
            "shard_export_rows": lambda: L.gamma_hip_ivfpq_shard_export_rows(h, a, 4, p, C.byref(mx)),
            "shard_export": lambda: L.gamma_hip_ivfpq_shard_export(h, a, 4, p, p, p, 64, p, p, p),
            "shard_export_exact": lambda: L.gamma_hip_ivfpq_shard_export_exact(h, a, 4, p, p, p, p, 64, p, p),
            "merge_replay": lambda: L.gamma_hip_ivfpq_merge_replay(h, a, 1, 4, p, 64, p, p, p, 10, p, p, p),
            "merge_replay_exact": lambda: L.gamma_hip_ivfpq_merge_replay_exact(h, a, 1, 4, p, 64, p, p, p, p, 10, p, p, p),
            "set_list_mask": lambda: L.gamma_hip_ivfpq_set_list_mask(h, np.ones(16, np.uint8).ctypes.data_as(C.POINTER(C.c_uint8))),
        }
        for name, fn in calls.items():
            rc = fn()
            msg = L.gamma_hip_last_error(h).decode()
            assert rc == -6, (name, rc, msg)          # GAMMA_HIP_EUNSUPPORTED
            assert "4-bit handle" in msg and "8-bit only" in msg, (name, msg)
    finally:
        g.close()
    # a precomputed table beyond precomputed_table_max_bytes (table mode 0): refused at init, with a message
    old = api.get_precomputed_table_max_bytes()
    g = api.GammaHip(0)
    try:
        api.set_precomputed_table_max_bytes(16 * 8 * 16 * 4 - 1)
        with pytest.raises(api.GammaHipError, match="precomputed_table_max_bytes"):
            g.ivfpq4_init(32, 16, 8)
    finally:
        api.set_precomputed_table_max_bytes(old)
        g.close()
    # the 8-bit init keeps refusing nbits = 4; bad shapes are refused by the 4-bit one
    g = api.GammaHip(0)
    try:
        with pytest.raises(api.GammaHipError):
            g.ivfpq_init(16, 8, 4, nbits=4)
        with pytest.raises(api.GammaHipError):
            g.ivfpq4_init(30, 8, 4)          # d % M != 0
        with pytest.raises(api.GammaHipError):
            g.ivfpq4_init(258, 8, 129)       # code_size > 64
        g.ivfpq4_init(16, 8, 4)
        with pytest.raises(api.GammaHipError):
            g.ivfpq_search(np.zeros((1, 16), np.float32), 1, api.SearchArgs(nprobe=1))   # not trained
    finally:
        g.close()


def test_8bit_handle_beside_a_4bit_one():
    case = fixtures.trained_case(d=32, nlist=32, M=8, N=6000, nq=24, metric=B.METRIC_L2)
    c, ix = _case(32, 16, 8)
    g4 = _handle(c)
    g8 = fixtures.load_hip(case, device=0)
    try:
        q4 = PR.clustered(24, 32, 71)
        ctx = B.make_ctx(min_score=-3e38, max_score=3e38)
        args = api.SearchArgs(metric=api.METRIC_L2, nprobe=8, recall_num=64, has_rank=True, **WIDE)
        for _ in range(2):
            _check(g4, ix, q4, 10, 6, 50)
            D, I = case["oracle"].search(case["q"], 10, 8, recall_num=64, has_rank=True, metric=B.METRIC_L2, ctx=ctx)
            Dg, Ig = g8.ivfpq_search(case["q"], 10, args)
            compare_exact(D, I, Dg, Ig)
        assert g8.code_size() == 8 and g4.code_size() == 4
    finally:
        g4.close()
        g8.close()
