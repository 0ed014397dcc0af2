"""GPU: the OPQ rotation on a handle (gamma_hip_opq_set / _get / _apply / _apply_device) against tests/opq_ref.py.

The rotation itself is compared bit for bit with the contract's chain (apply_chain) and bounded against the float64
product; everything downstream -- lists after Add / Update, the three stages of every search -- is compared strictly
with the CPU oracle over the rotated base, the exact re-rank being done on the raw vectors."""
import ctypes as C

import numpy as np
import pytest

from gamma_amd import _lib, api
from oracle import binding as B
from tests import fixtures
from tests import opq_ref as OR
from tests.parity import compare_exact, compare_search_exact

pytestmark = pytest.mark.gpu

SHAPES = [(32, 16, 8), (128, 32, 16), (20, 16, 5), (15, 8, 5), (160, 16, 16)]   # (d, nlist, M); 15: the VALU chain
IDS = lambda s: "d%d_l%d_m%d" % s
N = 4000
EUNSUPPORTED = -6
EINVAL = -1
_cases = {}


def _empty_handle(d, nlist, M, metric=api.METRIC_L2, A=None):
    g = api.GammaHip(0)
    g.ivfpq_init(d, nlist, M, 8, metric)
    if A is not None:
        g.opq_set(A)
    return g


def _case(d, nlist, M, metric=api.METRIC_L2):
    """raw base, rotation, the base rotated by the device (bit-equal to apply_chain: test_rotation_bits) and the oracle
    over it, built once per shape and left unchanged"""
    key = (d, nlist, M, metric)
    if key not in _cases:
        A = OR.random_rotation(d, 100 + d)
        base = OR.clustered(N, d, 5)
        g = _empty_handle(d, nlist, M, metric, A)
        try:
            base_rot = g.opq_apply(base)
        finally:
            g.close()
        o, cc, pq = OR.build_oracle(base_rot, nlist, M, metric)
        _cases[key] = dict(d=d, nlist=nlist, M=M, metric=metric, A=A, base=base, base_rot=base_rot, o=o, cc=cc, pq=pq)
    return _cases[key]


def _handle(c, add=True):
    g = _empty_handle(c["d"], c["nlist"], c["M"], c["metric"], c["A"])
    g.ivfpq_set_trained(c["cc"], c["pq"], None)
    g.raw_init(c["d"])
    g.raw_append(c["base"])
    if add:
        g.add(c["base"], 0)
    return g


def _assert_lists(g, o, nlist, what):
    for l in range(nlist):
        ids, cds = g.get_list(l)
        oi, oc = o.get_list(l)
        assert np.array_equal(ids, oi) and cds.tobytes() == oc.tobytes(), "%s: list %d" % (what, l)


# ---- the rotation ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_rotation_bits_and_accuracy(shape):
    d, nlist, M = shape
    rng = np.random.default_rng(d)
    for A in (OR.random_rotation(d, 7 + d), OR.mixed_magnitude(d, 8 + d)):
        g = _empty_handle(d, nlist, M, A=A)
        try:
            for n in (1, 33, 65, 700):
                x = (rng.standard_normal((n, d)) * 10.0 ** rng.uniform(-2, 2, (n, 1))).astype(np.float32)
                xt = g.opq_apply(x)
                ref = OR.apply_chain(A, x)
                assert xt.tobytes() == ref.tobytes(), "d=%d n=%d: %d elements differ from the chain" % (
                    d, n, int((xt.view(np.uint32) != ref.view(np.uint32)).sum()))
                exact = x.astype(np.float64) @ A.astype(np.float64).T
                assert (np.abs(xt.astype(np.float64) - exact) <= OR.chain_bound(A, x)).all()
        finally:
            g.close()


def test_rotation_is_independent_of_the_batch():
    import torch
    d = 128
    A = OR.random_rotation(d, 3)
    x = OR.clustered(700, d, 9)
    for dd, AA, xx in ((d, A, x), (15, OR.random_rotation(15, 4), OR.clustered(700, 15, 10))):
        g = _empty_handle(dd, 8, 5 if dd == 15 else 16, A=AA)
        try:
            whole = g.opq_apply(xx)
            for i in (0, 1, 31, 32, 63, 64, 699):
                assert g.opq_apply(xx[i:i + 1]).tobytes() == whole[i:i + 1].tobytes(), "row %d alone" % i
            for off in (1, 3, 33, 64, 650):
                assert g.opq_apply(xx[off:]).tobytes() == whole[off:].tobytes(), "offset %d" % off
            # device pointers on the handle's stream give the same bytes
            tx = torch.from_numpy(xx).cuda()
            tt = torch.empty_like(tx)
            g.opq_apply_device(tx.data_ptr(), len(xx), tt.data_ptr())
            g.synchronize()
            assert tt.cpu().numpy().tobytes() == whole.tobytes()
        finally:
            g.close()


# ---- the handle's contract -------------------------------------------------------------------------------------------
def test_set_get_and_when_set_is_allowed():
    c = _case(32, 16, 8)
    g = _empty_handle(32, 16, 8)
    try:
        assert g.opq_get() is None
        L = g.L
        x = np.zeros((1, 32), np.float32)
        assert L.gamma_hip_opq_apply(g.h, 1, x.ctypes.data_as(_lib.f32p), x.ctypes.data_as(_lib.f32p)) == EINVAL
        g.opq_set(c["A"])
        assert g.opq_get().tobytes() == c["A"].tobytes()
        A2 = OR.mixed_magnitude(32, 1)
        g.opq_set(A2)                                  # still empty: may be replaced
        assert g.opq_get().tobytes() == A2.tobytes()
        g.opq_set(c["A"])
        g.ivfpq_set_trained(c["cc"], c["pq"], None)
        g.add(c["base"][:100], 0)
        rc = L.gamma_hip_opq_set(g.h, c["A"].ctypes.data_as(_lib.f32p))
        assert rc == EINVAL and b"hold entries" in L.gamma_hip_last_error(g.h)
    finally:
        g.close()


def test_set_is_refused_on_other_models_and_group_members():
    A = OR.random_rotation(32, 1)
    pA = A.ctypes.data_as(_lib.f32p)

    def refused(g):
        rc = g.L.gamma_hip_opq_set(g.h, pA)
        msg = g.L.gamma_hip_last_error(g.h)
        assert rc == EUNSUPPORTED and b"opq_set" in msg, (rc, msg)
        assert g.L.gamma_hip_opq_get(g.h, None) == 0

    g = api.GammaHip(0)
    try:
        g.ivfpq4_init(32, 16, 8)
        refused(g)
    finally:
        g.close()
    g = api.GammaHip(0)
    try:
        g.ivfflat_init(32, 16)
        refused(g)
    finally:
        g.close()
    g = api.GammaHip(0)
    try:
        g.binivf_init(32, 16)
        refused(g)
    finally:
        g.close()
    g = api.GammaHip(0)
    try:
        g.ivfpq_init(32, 16, 8)
        g.set_list_mask(np.ones(16, np.uint8))
        refused(g)                                     # a list shard
    finally:
        g.close()
    grp = api.GammaHipGroup([0, 0])
    try:
        grp.members[0].ivfpq_init(32, 16, 8)
        refused(grp.members[0])
    finally:
        grp.close()


REFUSED = ["gamma_hip_ivfpq_search_shard", "gamma_hip_ivfpq_coarse_device", "gamma_hip_ivfpq_search_shard_preassigned",
           "gamma_hip_ivfpq_search_shard_bounded", "gamma_hip_ivfpq_merge_rerank", "gamma_hip_ivfpq_merge_rerank_exact",
           "gamma_hip_ivfpq_shard_exact", "gamma_hip_ivfpq_shard_export_exact", "gamma_hip_ivfpq_shard_cut_flags",
           "gamma_hip_ivfpq_merge_set_shard_flags", "gamma_hip_ivfpq_merge_flagged", "gamma_hip_ivfpq_shard_export_rows",
           "gamma_hip_ivfpq_shard_export", "gamma_hip_ivfpq_merge_replay", "gamma_hip_ivfpq_merge_replay_exact",
           "gamma_hip_ivfpq_set_list_mask"]


def test_entries_that_do_not_rotate_refuse_a_handle_with_a_matrix():
    import torch
    c = _case(32, 16, 8)
    g = _handle(c)
    keep = []
    try:
        buf = torch.zeros(1 << 16, dtype=torch.float32, device="cuda")   # every pointer argument: valid device memory
        sa = api.SearchArgs(metric=api.METRIC_L2, nprobe=4, recall_num=20)

        def arg(t):
            if t is C.c_void_p:
                return C.c_void_p(buf.data_ptr())
            if t is C.c_int:
                return 4
            if t is C.c_int64:
                return 8
            if t is C.POINTER(_lib.SearchParams):
                return sa.ref()
            if t is _lib.u8p:
                a = np.ones(64, np.uint8)
                keep.append(a)
                return a.ctypes.data_as(_lib.u8p)
            obj = t._type_()                           # out parameters: a word of the pointed-to type
            keep.append(obj)
            return C.byref(obj)

        for name in REFUSED:
            _, argtypes = _lib.SYMBOLS[name]
            a = [arg(t) for t in argtypes[1:]]
            if name == "gamma_hip_ivfpq_search_shard_bounded":
                a[-2:] = [None, None]                  # no reduce callback
            rc = getattr(g.L, name)(g.h, *a)
            msg = g.L.gamma_hip_last_error(g.h)
            assert rc == EUNSUPPORTED and b"OPQ" in msg, (name, rc, msg)
        g.synchronize()
    finally:
        g.close()


# ---- lists -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_lists_after_add_encode_and_update(shape):
    d, nlist, M = shape
    c = _case(d, nlist, M)
    g = _handle(c)
    try:
        _assert_lists(g, c["o"], nlist, "add")
        B.lib().go_set_assign_mode(-1)
        for n in (300, 7):                             # the GEMM form, and below 20 vectors the exact form
            lno, codes = g.encode(c["base"][:n])
            rl, rc = c["o"].encode(c["base_rot"][:n])
            assert np.array_equal(lno, rl) and codes.tobytes() == rc.tobytes(), "encode n=%d" % n
        # _encode_each: every vector assigned as a call of its own
        n = 40
        lno = np.empty(n, np.int64)
        codes = np.empty((n, M), np.uint8)
        x = np.ascontiguousarray(c["base"][:n])
        assert g.L.gamma_hip_ivfpq_encode_each(g.h, n, x.ctypes.data_as(_lib.f32p), lno.ctypes.data_as(_lib.i64p),
                                               codes.ctypes.data_as(_lib.u8p)) == 0
        B.lib().go_set_assign_mode(0)
        rl, rc = c["o"].encode(c["base_rot"][:n])
        B.lib().go_set_assign_mode(-1)
        assert np.array_equal(lno, rl) and codes.tobytes() == rc.tobytes(), "encode_each"
    finally:
        g.close()
    # Update on an oracle of its own (the shared one stays as it is)
    o2 = B.OracleIVFPQ(d, nlist, M, 8, c["metric"])
    o2.set_trained(c["cc"], c["pq"], None)
    B.lib().go_set_assign_mode(-1)
    assert o2.add(c["base_rot"])
    g = _handle(c)
    try:
        rng = np.random.default_rng(d)
        for n in (1, 50):
            vids = rng.choice(N, n, replace=False).astype(np.int64)
            vecs = OR.clustered(n, d, 70 + n)
            rot = g.opq_apply(vecs)
            g.update_batch(vids, vecs)
            for v, r in zip(vids, rot):
                o2.update(int(v), r[None, :])
            _assert_lists(g, o2, nlist, "update n=%d" % n)
    finally:
        g.close()


# ---- searches --------------------------------------------------------------------------------------------------------
def _check(g, c, q, k, P, R, has_rank, metric, entry="host", stages=True, **kw):
    import torch
    fk = {}
    ak = {}
    if "deleted" in kw:
        bm = np.zeros((N + 7) // 8, np.uint8)
        np.bitwise_or.at(bm, kw["deleted"] >> 3, (1 << (kw["deleted"] & 7)).astype(np.uint8))
        fk["docids_bitmap"] = bm
    if "docs" in kw:
        fk["range_filters"] = [B.make_range_filter(kw["docs"])]
        ak["range_filters"] = [api.make_range_filter(kw["docs"])]
    lo, hi = kw.get("lo", -3e38), kw.get("hi", 3e38)
    # q is a stream: the first nq of its vectors that meet the yardstick's condition on the inputs (decided on the CPU)
    q = OR.pick_queries(c["o"], c["base"], c["A"], q, kw.get("nq", max(1, len(q) * 7 // 8)), k, P, R, metric, **fk)
    q_rot = g.opq_apply(q)
    D, I, st = OR.search_ref(c["o"], c["base"], q, q_rot, k, P, R, has_rank, metric, min_score=lo, max_score=hi, **fk)
    args = api.SearchArgs(metric=metric, nprobe=P, recall_num=R, has_rank=has_rank, min_score=lo, max_score=hi, **ak)
    if entry == "host":
        Dg, Ig = g.ivfpq_search(q, k, args)
    else:
        tq = torch.from_numpy(q).cuda()
        tD = torch.empty((len(q), k), dtype=torch.float32, device="cuda")
        tI = torch.empty((len(q), k), dtype=torch.int64, device="cuda")
        if entry == "device":
            g.ivfpq_search_device(tq.data_ptr(), len(q), k, args, tD.data_ptr(), tI.data_ptr())
            g.synchronize()
        else:
            g.ivfpq_search_device_wait(tq.data_ptr(), len(q), k, args, tD.data_ptr(), tI.data_ptr())
        Dg, Ig = tD.cpu().numpy(), tI.cpu().numpy()
    if stages:
        compare_search_exact(D, I, st, Dg, Ig, g.last_stages(len(q), P, max(R, k)))
    else:                                              # a call of several chunks leaves the stages of its last chunk only
        compare_exact(D, I, Dg, Ig)
    return Dg, Ig


@pytest.mark.parametrize("metric", [api.METRIC_L2, api.METRIC_IP], ids=["L2", "IP"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_searches(shape, metric):
    d, nlist, M = shape
    c = _case(d, nlist, M, metric)
    g = _handle(c)
    try:
        P = min(5, nlist)
        for nq in (1, 8, 25, 700):                     # small chain with exact / GEMM-form coarse step; regular chain
            q = OR.clustered(nq + 40, d, 200 + nq)
            for has_rank in (True, False):
                _check(g, c, q, 10, P, 40, has_rank, metric, nq=nq)
        g.set_dist_budget(1 << 20)                     # the 700 queries again as a call of several chunks
        assert (1 << 20) // (P * g.max_list_len() * 4) < 350
        for has_rank in (True, False):
            _check(g, c, q, 10, P, 40, has_rank, metric, stages=False, nq=700)
        g.set_dist_budget(8 << 30)
        # the other metric as a per-request metric
        other = api.METRIC_IP if metric == api.METRIC_L2 else api.METRIC_L2
        _check(g, c, OR.clustered(40, d, 31), 10, P, 40, True, other, nq=25)
        assert g.ties_not_honoured() == 0
    finally:
        g.close()


def test_regular_chain_on_small_batches_filters_window_and_entries():
    c = _case(32, 16, 8)
    g = _handle(c)
    try:
        rng = np.random.default_rng(2)
        g.set_small_path(False)                        # the regular chain with the exact and the GEMM-form coarse step
        for nq in (8, 25):
            for has_rank in (True, False):
                _check(g, c, OR.clustered(nq + 20, 32, 300 + nq), 10, 5, 40, has_rank, api.METRIC_L2, nq=nq)
        g.set_small_path(True)
        q = OR.clustered(60, 32, 6)
        # the three entries return the same bytes
        outs = [_check(g, c, q, 10, 5, 40, True, api.METRIC_L2, entry=e, nq=48) for e in ("host", "device", "device_wait")]
        for Dg, Ig in outs[1:]:
            assert Dg.tobytes() == outs[0][0].tobytes() and np.array_equal(Ig, outs[0][1])
        # a narrow score window: on the exact distance with has_rank, on the ADC distance without
        D = outs[0][0]
        lo, hi = float(np.median(D[:, 2])), float(np.median(D[:, 7]))
        for has_rank in (True, False):
            _check(g, c, q, 10, 5, 40, has_rank, api.METRIC_L2, lo=lo, hi=hi, nq=48)
        # deleted docs and a range filter, small and large batch
        deleted = rng.choice(N, N // 5, replace=False)
        docs = rng.choice(N, N // 2, replace=False)
        g.bitmap_set(deleted)
        g.delete(deleted)
        for qq, nq in ((q, 48), (OR.clustered(740, 32, 61), 700)):
            for has_rank in (True, False):
                _check(g, c, qq, 10, 5, 40, has_rank, api.METRIC_L2, deleted=deleted, docs=docs, nq=nq)
    finally:
        g.close()


def test_exact_ties_end_to_end():
    """integer-valued data and a signed permutation: the rotation and every distance are exact in fp32 in any order, so an
    oracle that holds the ROTATED base as its raw store and is asked the rotated queries is the complete expected result,
    ties at the nprobe, recall_num and k cuts included"""
    d, nlist, M = 32, 16, 8
    rng = np.random.default_rng(11)
    A = OR.signed_permutation(d, 5)
    distinct = rng.integers(-8, 9, (N // 4, d)).astype(np.float32)
    base = distinct[rng.permutation(np.repeat(np.arange(N // 4), 4))]     # every vector four times: equal codes, equal distances
    q = np.concatenate([rng.integers(-8, 9, (40, d)).astype(np.float32), base[:24]])
    base_rot, q_rot = OR.apply_chain(A, base), OR.apply_chain(A, q)
    assert np.array_equal(base_rot, base.astype(np.float64) @ A.astype(np.float64).T)
    for metric in (api.METRIC_L2, api.METRIC_IP):
        o, cc, pq = OR.build_oracle(base_rot, nlist, M, metric, raw=base_rot)
        g = _empty_handle(d, nlist, M, metric, A)
        try:
            g.ivfpq_set_trained(cc, pq, None)
            g.raw_init(d)
            g.raw_append(base)
            g.add(base, 0)
            g.set_exact_ties(True)
            _assert_lists(g, o, nlist, "add")
            for nq in (8, 64):
                for has_rank in (True, False):
                    for P, R, k in ((4, 30, 10), (3, 10, 10)):
                        ctx = B.make_ctx(min_score=-3e38, max_score=3e38)
                        D, I, st = o.search(q_rot[:nq], k, P, recall_num=R, has_rank=has_rank, metric=metric, ctx=ctx,
                                            want_stages=True)
                        args = api.SearchArgs(metric=metric, nprobe=P, recall_num=R, has_rank=has_rank, min_score=-3e38,
                                              max_score=3e38)
                        Dg, Ig = g.ivfpq_search(q[:nq], k, args)
                        compare_search_exact(D, I, st, Dg, Ig, g.last_stages(nq, P, max(R, k)))
            assert g.tie_stats()["replayed"] > 0, "no query was replayed: the data has no ties at a cut"
            assert g.ties_not_honoured() == 0
        finally:
            g.close()


# ---- a handle without a matrix ---------------------------------------------------------------------------------------
def test_handle_without_a_matrix_is_unchanged():
    case = fixtures.trained_case(d=32, nlist=32, M=8, N=6000, nq=24, metric=B.METRIC_L2)
    g = fixtures.load_hip(case, device=0)
    try:
        assert g.opq_get() is None
        ctx = B.make_ctx(min_score=-1e30, max_score=1e30)
        for has_rank in (True, False):
            D, I, st = case["oracle"].search(case["q"], 10, 8, recall_num=64, has_rank=has_rank, metric=B.METRIC_L2, ctx=ctx,
                                             want_stages=True)
            args = api.SearchArgs(metric=api.METRIC_L2, nprobe=8, recall_num=64, has_rank=has_rank, min_score=-1e30,
                                  max_score=1e30)
            Dg, Ig = g.ivfpq_search(case["q"], 10, args)
            compare_search_exact(D, I, st, Dg, Ig, g.last_stages(24, 8, 64))
    finally:
        g.close()
