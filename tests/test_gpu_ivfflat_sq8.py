"""GPU: IVFFLAT search over a scalar-quantised raw store (gamma_hip_set_ivfflat_sq8_rows).

The store is lossy and nothing else is: it holds W = sq8_ref.stored(base, vmin, vmax), a code is decoded as it is loaded (a
multiply, then an add, each rounded in fp32) and every distance is fvec_L2sqr / fvec_inner_product of the fp32 query and the
decoded row.  So the results must be
  * the CPU oracle's IVFFLAT search over the same lists with set_raw(W), labels and distance bits at every rank (compare_exact,
    exact ties on), and
  * byte-identical to those of a second handle whose fp32 store holds W and whose lists are the same.
Every check also reads the handles' path counters (ivfflat_scan_stats): the case ran the kernel it is named for and no other.
nlist = 16 and N = 3001 (lists of about 190 rows: one full 128-row chunk and a partial one) are the smallest shapes at which each
of the scan's launch sites can go wrong (the rules: ivfflat_search_device_locked).  The data comes from
tests/ivfflat_sq8_data.py, whose properties tests/test_ivfflat_sq8_cpu.py checks on the CPU."""
import numpy as np
import pytest

from gamma_amd import _lib, api
from oracle import binding as B
from tests import ivfflat_sq8_data as Q
from tests import sq8_ref as S
from tests.parity import compare_exact, compare_topk

pytestmark = pytest.mark.gpu

WIDE = dict(min_score=-3e38, max_score=3e38)
EUNSUPPORTED = -6   # include/gamma_hip.h
L2, IP = B.METRIC_L2, B.METRIC_IP
SMALL, PAIR, FIXED, SLICED = 0, 1, 2, 3      # ivfflat_scan_stats


def bitmap_of(n, dead):
    bm = np.zeros((n >> 3) + 1, dtype=np.uint8)
    np.bitwise_or.at(bm, dead >> 3, (1 << (dead & 7)).astype(np.uint8))
    return bm


def sq8_handle(c):
    g = api.GammaHip(0)
    g.ivfflat_init(c.d, c.nlist, c.metric)
    g.ivfflat_set_trained(c.cc)
    c.load(g)
    g.raw_init(c.d, "sq8")
    g.raw_sq8_set_ranges(c.vmin, c.vmax)
    g.raw_append(c.base)
    return g


class Pair:
    """the sq8 store under test (fed the caller's rows, which it encodes) and the fp32 store of the rows it holds, W, both behind
    the lists of the case"""

    def __init__(self, case, small_path=None, mask=False):
        self.c = case
        self.g = sq8_handle(case)
        self.g.set_ivfflat_sq8_rows(True)
        self.g32 = api.GammaHip(0)
        self.g32.ivfflat_init(case.d, case.nlist, case.metric)
        self.g32.ivfflat_set_trained(case.cc)
        case.load(self.g32)
        self.g32.raw_init(case.d)
        self.g32.raw_append(case.W)
        for h in (self.g, self.g32):
            if small_path is not None:
                h.set_small_path(small_path)
            if mask:
                h.set_list_mask(np.ones(case.nlist, np.uint8))
        assert self.g.raw_elem_type() == 4 and self.g32.raw_elem_type() == 0

    def close(self):
        self.g.close()
        self.g32.close()

    def both(self, f):
        f(self.g)
        f(self.g32)

    def check(self, q, k, P, ran, win=WIDE, bm=None, docs=None, exact_ties=1):
        ctx_kw, kw = {}, {}
        if bm is not None:
            ctx_kw["docids_bitmap"] = bm
        if docs is not None:
            ctx_kw["range_filters"] = [B.make_range_filter(docs)]
            kw["range_filters"] = [api.make_range_filter(docs)]
        D, I = self.c.oracle(q, k, P, **win, **ctx_kw)
        args = api.SearchArgs(metric=self.c.metric, nprobe=P, exact_ties=exact_ties, **win, **kw)
        self.both(lambda h: h.ivfflat_scan_stats(reset=True))
        Dg, Ig = self.g.ivfflat_search(q, k, args)
        D32, I32 = self.g32.ivfflat_search(q, k, args)
        if exact_ties >= 0:
            compare_exact(D, I, Dg, Ig)
        else:      # exact ties off: the order inside a group of equal distances is the device's own
            compare_topk(D, I, Dg, Ig)
        assert Dg.tobytes() == D32.tobytes() and Ig.tobytes() == I32.tobytes()
        for h in (self.g, self.g32):      # which kernel scanned
            s = h.ivfflat_scan_stats()
            assert s[ran] > 0 and all(s[i] == 0 for i in range(4) if i != ran), (ran, s)
        return D, I

    def check_filtered(self, q, k, P, ran, seed):
        """delete bitmap + range filter + score window"""
        N = self.c.N
        rng = np.random.default_rng(seed)
        bm = bitmap_of(N, rng.choice(N, N // 7, replace=False))
        docs = rng.choice(N, 3 * N // 4, replace=False)
        self.both(lambda h: h.bitmap_upload(bm, N))
        Dw, Iw = self.check(q, k, P, ran, bm=bm, docs=docs)
        fin = Dw[Iw >= 0]
        win = dict(min_score=float(np.quantile(fin, 0.2)), max_score=float(np.quantile(fin, 0.9)))
        D, I = self.check(q, k, P, ran, win=win, bm=bm, docs=docs)
        assert D.tobytes() != Dw.tobytes()      # the window cut something

    def move_and_rewrite(self, src, dst):
        """a vector moves from list src to list dst, as an Update moves it: its old entry stays with bit 63 set and must be
        skipped; its row is rewritten through raw_write (the sq8 store encodes the caller's row, the fp32 store gets what that
        store then holds).  Returns (vid, the stored row)."""
        c = self.c
        step, inv = S.params(c.vmin, c.vmax)
        vid = int(c.lists[src][3])
        new = c.base[int(c.lists[dst][0])].copy()      # a neighbour of a row of dst: three steps away in one element
        code = int(S.encode(new[None], c.vmin, inv)[0, 1])
        new[1] += np.float32(3.0 if code < 128 else -3.0) * step[1]
        held = c.stored(new[None])
        assert step[1] > 0 and (held[0] != c.W[int(c.lists[dst][0])]).any()
        c.o.update_code(dst, vid, np.zeros(1, np.uint8))
        c.raw[vid] = held[0]
        self.both(lambda h: h.update(dst, vid, np.zeros(1, np.uint8)))
        self.g.raw_write(vid, new[None])
        self.g32.raw_write(vid, held)
        ids = self.g.get_list(src)[0]
        assert (ids < 0).sum() == 1 and np.array_equal(ids, c.o.get_list(src)[0])
        return vid, held[0]


# ---- the switch -------------------------------------------------------------------------------------------------------
def test_switch_turns_ivfflat_search_over_sq8_rows_on():
    """off (the default): EUNSUPPORTED with the sq8 store's refusal message, as before; each of the two other switches alone
    changes nothing; on: served; off again: refused again.  With the switch on, raw_put / raw_drop, the shard entry points and
    the flat search of the same handle still refuse."""
    import torch
    c = Q.Case(24, L2, N=700, nlist=4, nq=8, seed=1)
    g = sq8_handle(c)
    L = g.L
    args = api.SearchArgs(metric=api.METRIC_L2, nprobe=2, **WIDE)
    D = np.empty((8, 5), np.float32)
    I = np.empty((8, 5), np.int64)

    def search():
        return L.gamma_hip_ivfflat_search(g.h, args.ref(), 8, c.q.ctypes.data_as(_lib.f32p), 5, D.ctypes.data_as(_lib.f32p),
                                          I.ctypes.data_as(_lib.i64p))

    def refused(rc, what=b"reads fp32 rows"):
        msg = L.gamma_hip_last_error(g.h)
        assert rc == EUNSUPPORTED and b"sq8" in msg and b"gamma_hip_raw_init_sq8" in msg and what in msg, (rc, msg)

    try:
        refused(search(), b"IVFFLAT search reads fp32 rows")
        g.set_ivfflat_narrow_rows(True)      # the other narrow stores' switch: not this store's
        refused(search(), b"IVFFLAT search reads fp32 rows")
        g.set_ivfflat_narrow_rows(False)
        g.set_flat_sq8_rows(True)            # the flat search's switch: not this search's
        refused(search(), b"IVFFLAT search reads fp32 rows")
        g.set_flat_sq8_rows(False)
        g.set_ivfflat_sq8_rows(True)
        assert search() == 0
        compare_exact(*c.oracle(c.q, 5, 2, **WIDE), D, I)
        vids = np.arange(4, dtype=np.int64)
        refused(L.gamma_hip_raw_put(g.h, 4, vids.ctypes.data_as(_lib.i64p), c.base[:4].ctypes.data_as(_lib.f32p)), b"")
        refused(L.gamma_hip_raw_drop(g.h, 4, vids.ctypes.data_as(_lib.i64p)), b"")
        tq = torch.from_numpy(c.q).cuda()
        tids = torch.zeros((8, 50), dtype=torch.int64, device="cuda")
        tex = torch.full((8, 50), 1.0, dtype=torch.float32, device="cuda")
        toff = torch.zeros((8, 64), dtype=torch.int32, device="cuda")
        refused(L.gamma_hip_ivfpq_shard_exact(g.h, args.ref(), 8, tq.data_ptr(), tids.data_ptr(), 50, tex.data_ptr()), b"")
        refused(L.gamma_hip_ivfpq_shard_export_exact(g.h, args.ref(), 8, tq.data_ptr(), tex.data_ptr(), tids.data_ptr(),
                                                     toff.data_ptr(), 50, tex.data_ptr(), tex.data_ptr()), b"")
        # the switch is IVFFLAT's alone: the flat search of the same handle still refuses
        refused(L.gamma_hip_flat_search(g.h, args.ref(), 8, c.q.ctypes.data_as(_lib.f32p), 5, D.ctypes.data_as(_lib.f32p),
                                        I.ctypes.data_as(_lib.i64p)), b"flat search reads fp32 rows")
        g.set_ivfflat_sq8_rows(False)
        refused(search(), b"IVFFLAT search reads fp32 rows")
    finally:
        g.close()


@pytest.mark.parametrize("dtype", ["float32", "uint8"])
def test_switch_leaves_the_other_stores_alone(dtype):
    """an fp32 store, and a uint8 store behind gamma_hip_set_ivfflat_narrow_rows, answer byte for byte the same with the new
    switch on and off (list-major and small path); the uint8 store without ITS switch stays refused whatever the new one says"""
    from tests import ivfflat_rows_data as R
    c = R.Case(32, "uint8", L2, N=900, nlist=4, nq=40, seed=2)
    g = api.GammaHip(0)
    try:
        g.ivfflat_init(c.d, c.nlist, api.METRIC_L2)
        g.ivfflat_set_trained(c.cc)
        c.load(g)
        g.raw_init(c.d, dtype)
        g.raw_append(c.W)
        args = api.SearchArgs(metric=api.METRIC_L2, nprobe=2, **WIDE)
        if dtype == "uint8":
            g.set_ivfflat_sq8_rows(True)
            with pytest.raises(Exception):
                g.ivfflat_search(c.q, 5, args)
            g.set_ivfflat_sq8_rows(False)
            g.set_ivfflat_narrow_rows(True)
        res = []
        for on in (False, True, False):
            g.set_ivfflat_sq8_rows(on)
            for nq in (40, 3):      # list-major | the small path
                res.append(g.ivfflat_search(c.q[:nq], 5, args))
        for i in (2, 4):
            assert res[i][0].tobytes() == res[0][0].tobytes() and res[i][1].tobytes() == res[0][1].tobytes()
            assert res[i + 1][0].tobytes() == res[1][0].tobytes() and res[i + 1][1].tobytes() == res[1][1].tobytes()
        compare_exact(*c.oracle(c.q, 5, 2, **WIDE), *res[2])
    finally:
        g.close()


# ---- the list-major kernel (ivfflat.hip k_ivfflat_lm) -------------------------------------------------------------------
# 33 queries x 4 probes = 132 pairs >= 2 nlist, d in {16, 32, 64, 96, 128}, no list mask: list-major.  Lists of about 190 rows:
# a full 128-row chunk and a partial one.  With 16 probes every list is probed by all 33 queries: a second, partial query tile.
@pytest.mark.parametrize("metric", [L2, IP], ids=["l2", "ip"])
@pytest.mark.parametrize("d", [16, 32, 64, 96, 128])
def test_list_major_kernel_over_sq8_rows(d, metric):
    """list 5 is empty, and probed by every query of the 16-probe call.  Then a vector moves to another list: its old entry
    keeps bit 63 and is skipped, its row is rewritten through raw_write and the search sees the new row."""
    c = Q.Case(d, metric, empty=5, seed=d)
    assert (c.W != c.base).any()
    p = Pair(c)
    try:
        p.check(c.q, 10, 4, FIXED)
        p.check(c.q, 1, 16, FIXED)
        src = max(range(c.nlist), key=lambda l: len(c.lists[l]))
        dst = (src + 1) % c.nlist if (src + 1) % c.nlist != 5 else (src + 2) % c.nlist
        vid, held = p.move_and_rewrite(src, dst)
        q = np.concatenate([c.q, held[None]])      # the last query sits on the rewritten row
        D, I = p.check(q, 10, 4, FIXED)
        if metric == L2:
            assert I[-1, 0] == vid and D[-1, 0] == 0
        D, I = p.check(q[-2:], 10, 4, SMALL)      # 8 pairs: the small path over the same state
        if metric == L2:
            assert I[-1, 0] == vid
    finally:
        p.close()


# ---- the row-sliced kernel (ivfflat.hip k_ivfflat_lms) ----------------------------------------------------------------------
# 48 = the 32 + 16 pieces only; 144 = one slab + 16; 272 = two slabs + 16; 768 = six slabs.  With 16 probes every list is probed
# by all 33 queries: two full tiles of 16 and a tile of one.
@pytest.mark.parametrize("metric", [L2, IP], ids=["l2", "ip"])
@pytest.mark.parametrize("d", [48, 144, 272, 768])
def test_sliced_kernel_over_sq8_rows(d, metric):
    assert api.ivfflat_lm_shape(d)[0] == 2
    c = Q.Case(d, metric, seed=d)
    p = Pair(c)
    try:
        p.check(c.q, 10, 4, SLICED)
        p.check(c.q, 1, 16, SLICED)
    finally:
        p.close()


def test_sliced_kernel_lists_of_128_and_129_rows_an_empty_list_and_a_superseded_entry():
    c = Q.edge_case()
    assert [len(c.lists[l]) for l in (Q.EDGE_128, Q.EDGE_129, Q.EDGE_EMPTY)] == [128, 129, 0]
    p = Pair(c)
    try:
        p.check(c.q, 10, 4, SLICED)
        vid, held = p.move_and_rewrite(Q.EDGE_128, Q.EDGE_129)      # 128 entries, one of them dead; the other grows to 130
        assert len(p.g.get_list(Q.EDGE_128)[0]) == 128
        q = np.concatenate([c.q, held[None]])
        D, I = p.check(q, 10, 4, SLICED)
        assert I[-1, 0] == vid and D[-1, 0] == 0
    finally:
        p.close()


# ---- the pair kernel (rerank.hip k_ivfflat_scan), chunked path ---------------------------------------------------------
# d = 20, 33, 100 have no list-major form: 40 queries x 4 probes go to one workgroup per pair.  d = 33: byte loads; d = 20 and
# 100: dword loads, 100 with the four-element tail of rerank_dist8_sq8.
@pytest.mark.parametrize("d", [20, 33, 100])
def test_pair_kernel_over_sq8_rows(d):
    for metric in (L2, IP):
        c = Q.Case(d, metric, nq=40, seed=d)
        p = Pair(c)
        try:
            p.check(c.q, 10, 4, PAIR)
        finally:
            p.close()


def test_pair_kernel_at_d_128_below_the_list_major_threshold():
    """7 queries x 4 probes = 28 pairs < 2 nlist with the small path off: the chunked path's pair kernel at a d that has a
    list-major form (16-byte row loads, eight chunks in front of the chain)"""
    c = Q.Case(128, L2, nq=7, seed=5)
    p = Pair(c, small_path=False)
    try:
        p.check(c.q, 10, 4, PAIR)
        p.check(c.q[:1], 100, 4, PAIR)
    finally:
        p.close()


def test_a_call_under_a_list_mask_goes_to_the_pair_kernel():
    """a list mask that owns every list: the same results, scanned per pair although the shape is list-major's"""
    c = Q.Case(128, L2, seed=8)
    p = Pair(c, mask=True)
    try:
        p.check(c.q, 10, 4, PAIR)
    finally:
        p.close()


# ---- the small path (ivfflat_small) -------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,metric", [(128, L2), (33, IP), (64, IP), (20, L2)])
def test_small_path_over_sq8_rows(d, metric):
    """1 and 7 queries x 4 probes: fewer pairs than 2 nlist, small path on (the default)"""
    c = Q.Case(d, metric, nq=7, seed=6)
    p = Pair(c, small_path=True)
    try:
        for nq in (1, 7):
            p.check(c.q[:nq], 10, 4, SMALL)
            p.check(c.q[:nq], 300, 4, SMALL)
    finally:
        p.close()


# ---- filters ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,ran", [(64, FIXED), (144, SLICED), (100, PAIR)], ids=["list_major", "sliced", "pair"])
def test_delete_bitmap_range_filter_and_score_window(d, ran):
    c = Q.Case(d, L2, nq=40, seed=d + 1)
    p = Pair(c)
    try:
        p.check_filtered(c.q, 10, 4, ran, seed=d)
    finally:
        p.close()


# ---- exact ties -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,nq,ran", [(64, 33, FIXED), (144, 33, SLICED), (64, 7, SMALL), (100, 40, PAIR)],
                         ids=["list_major", "sliced", "small_path", "pair"])
def test_ties_at_the_k_cut_over_sq8_rows(d, nq, ran):
    """every row occurs four times, so ranks 8 .. 11 hold one distance and k = 10 cuts the group (shown with the oracle in
    tests/test_ivfflat_sq8_cpu.py): with exact ties on the survivors are the reference heap's, with them off the device's own --
    and the fp32 store's either way"""
    for metric in (L2, IP):
        c = Q.Case(d, metric, nq=nq, ties=True, seed=7)
        p = Pair(c)
        try:
            p.check(c.q, Q.TIE_K, 4, ran, exact_ties=1)
            p.check(c.q, Q.TIE_K, 4, ran, exact_ties=-1)
            if ran == SMALL:
                p.both(lambda h: h.set_small_path(False))      # the chunked path's tie replay, pair kernel
                p.check(c.q, Q.TIE_K, 4, PAIR, exact_ties=1)
        finally:
            p.close()


# ---- the device entry point --------------------------------------------------------------------------------------------
def test_device_entry_point_over_sq8_rows():
    """gamma_hip_ivfflat_search_device returns what the host entry returns (list-major and small path)"""
    import torch
    c = Q.Case(96, IP, seed=9)
    p = Pair(c)
    try:
        args = api.SearchArgs(metric=c.metric, nprobe=4, exact_ties=1, **WIDE)
        for nq, ran in ((33, FIXED), (5, SMALL)):
            D, I = p.check(c.q[:nq], 10, 4, ran)
            dx = torch.from_numpy(c.q[:nq]).cuda()
            dD = torch.empty((nq, 10), dtype=torch.float32, device="cuda")
            dI = torch.empty((nq, 10), dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            p.g.ivfflat_search_device(dx.data_ptr(), nq, 10, args, dD.data_ptr(), dI.data_ptr())
            p.g.synchronize()
            torch.cuda.synchronize()
            compare_exact(D, I, dD.cpu().numpy(), dI.cpu().numpy())
    finally:
        p.close()
