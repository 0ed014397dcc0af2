"""GPU: IVFFLAT search over a float16 / uint8 / int8 raw store (gamma_hip_set_ivfflat_narrow_rows).

A narrow row widens to fp32 exactly and every distance is fvec_L2sqr / fvec_inner_product of the fp32 query and the widened row,
so with W = base.astype(T).astype(float32) the results must be
  * the CPU oracle's IVFFLAT search over the same lists with set_raw(W), labels and distance bits at every rank (compare_exact,
    exact ties on), and
  * byte-identical to those of a second handle whose fp32 store holds W and whose lists are the same.
nlist = 16 and N = 3001 (lists of about 190 rows: two 128-row chunks, one partial) are the smallest shapes at which each of the
scan's three launch sites can go wrong; which site a case reaches is in its docstring (the rules: ivfflat_search_device_locked).
The data comes from tests/ivfflat_rows_data.py, whose properties tests/test_ivfflat_rows_cpu.py checks on the CPU."""
import numpy as np
import pytest

from gamma_amd import _lib, api
from oracle import binding as B
from tests import ivfflat_rows_data as R
from tests.parity import compare_exact, compare_topk

pytestmark = pytest.mark.gpu

WIDE = dict(min_score=-3e38, max_score=3e38)
DTYPES = R.DTYPES
EUNSUPPORTED = -6   # include/gamma_hip.h
L2, IP = B.METRIC_L2, B.METRIC_IP


def bitmap_of(n, dead):
    bm = np.zeros((n >> 3) + 1, dtype=np.uint8)
    np.bitwise_or.at(bm, dead >> 3, (1 << (dead & 7)).astype(np.uint8))
    return bm


class Pair:
    """the narrow store under test (fed the caller's rows, which it converts) and the fp32 store of the widened rows, both
    behind the lists of the case"""

    def __init__(self, case, small_path=None):
        self.c = case
        self.g, self.g32 = api.GammaHip(0), api.GammaHip(0)
        for h, dtype, rows in ((self.g, case.dtype, case.base), (self.g32, "float32", case.W)):
            h.ivfflat_init(case.d, case.nlist, case.metric)
            h.ivfflat_set_trained(case.cc)
            case.load(h)
            h.raw_init(case.d, dtype)
            h.raw_append(rows)
            if small_path is not None:
                h.set_small_path(small_path)
        self.g.set_ivfflat_narrow_rows(True)
        assert self.g.raw_elem_type() == 1 + DTYPES.index(case.dtype) and self.g32.raw_elem_type() == 0

    def close(self):
        self.g.close()
        self.g32.close()

    def both(self, f):
        f(self.g)
        f(self.g32)

    def check(self, q, k, P, win=WIDE, bm=None, docs=None, exact_ties=0):
        ctx_kw, kw = {}, {}
        if bm is not None:
            ctx_kw["docids_bitmap"] = bm
        if docs is not None:
            ctx_kw["range_filters"] = [B.make_range_filter(docs)]
            kw["range_filters"] = [api.make_range_filter(docs)]
        D, I = self.c.oracle(q, k, P, **win, **ctx_kw)
        args = api.SearchArgs(metric=self.c.metric, nprobe=P, exact_ties=exact_ties, **win, **kw)
        Dg, Ig = self.g.ivfflat_search(q, k, args)
        D32, I32 = self.g32.ivfflat_search(q, k, args)
        if exact_ties >= 0:
            compare_exact(D, I, Dg, Ig)
        else:      # exact ties off: the order inside a group of equal distances is the device's own
            compare_topk(D, I, Dg, Ig)
        assert Dg.tobytes() == D32.tobytes() and Ig.tobytes() == I32.tobytes()
        return D, I

    def check_filtered(self, q, k, P, seed):
        """delete bitmap + range filter + score window"""
        N = self.c.N
        rng = np.random.default_rng(seed)
        bm = bitmap_of(N, rng.choice(N, N // 7, replace=False))
        docs = rng.choice(N, 3 * N // 4, replace=False)
        self.both(lambda h: h.bitmap_upload(bm, N))
        Dw, Iw = self.check(q, k, P, bm=bm, docs=docs)
        fin = Dw[Iw >= 0]
        win = dict(min_score=float(np.quantile(fin, 0.2)), max_score=float(np.quantile(fin, 0.9)))
        D, I = self.check(q, k, P, win=win, bm=bm, docs=docs)
        assert D.tobytes() != Dw.tobytes()      # the window cut something


# ---- the switch -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_switch_turns_ivfflat_search_over_narrow_rows_on(dtype):
    """off (the default): EUNSUPPORTED with the store's refusal message, as before; the flat switch alone changes nothing; on:
    served; off again: refused again.  With the switch on raw_put still refuses the store."""
    c = R.Case(24, dtype, L2, N=700, nlist=4, nq=8, seed=1)
    word = b"float16" if dtype == "float16" else b"8-bit"
    g = api.GammaHip(0)
    L = g.L
    args = api.SearchArgs(metric=api.METRIC_L2, nprobe=2, **WIDE)
    D = np.empty((8, 5), np.float32)
    I = np.empty((8, 5), np.int64)

    def search():
        return L.gamma_hip_ivfflat_search(g.h, args.ref(), 8, c.q.ctypes.data_as(_lib.f32p), 5, D.ctypes.data_as(_lib.f32p),
                                          I.ctypes.data_as(_lib.i64p))

    def refused(rc, what=b"reads fp32 rows"):
        msg = L.gamma_hip_last_error(g.h)
        assert rc == EUNSUPPORTED and word in msg and what in msg, (rc, msg)

    try:
        g.ivfflat_init(c.d, c.nlist, api.METRIC_L2)
        g.ivfflat_set_trained(c.cc)
        c.load(g)
        g.raw_init(c.d, dtype)
        g.raw_append(c.base)
        refused(search())
        g.set_flat_narrow_rows(True)
        refused(search())
        g.set_flat_narrow_rows(False)
        g.set_ivfflat_narrow_rows(True)
        assert search() == 0
        compare_exact(*c.oracle(c.q, 5, 2, **WIDE), D, I)
        vids = np.arange(4, dtype=np.int64)
        refused(L.gamma_hip_raw_put(g.h, 4, vids.ctypes.data_as(_lib.i64p), c.W[:4].ctypes.data_as(_lib.f32p)),
                b"gamma_hip_raw_init_")      # (the store's own message: rows sharded with their lists are fp32)
        # the switch is IVFFLAT's alone: the flat search of the same handle still refuses
        refused(L.gamma_hip_flat_search(g.h, args.ref(), 8, c.q.ctypes.data_as(_lib.f32p), 5, D.ctypes.data_as(_lib.f32p),
                                        I.ctypes.data_as(_lib.i64p)))
        g.set_ivfflat_narrow_rows(False)
        refused(search())
    finally:
        g.close()


def test_switch_leaves_an_fp32_store_alone():
    c = R.Case(32, "int8", L2, N=900, nlist=4, nq=40, seed=2)
    g = api.GammaHip(0)
    try:
        g.ivfflat_init(c.d, c.nlist, api.METRIC_L2)
        g.ivfflat_set_trained(c.cc)
        c.load(g)
        g.raw_init(c.d)
        g.raw_append(c.W)
        res = []
        for on in (False, True, False):
            g.set_ivfflat_narrow_rows(on)
            for nq in (40, 3):      # list-major | the small path
                res.append(g.ivfflat_search(c.q[:nq], 5, api.SearchArgs(metric=api.METRIC_L2, nprobe=2, **WIDE)))
        for i in (2, 4):
            assert res[i][0].tobytes() == res[0][0].tobytes() and res[i][1].tobytes() == res[0][1].tobytes()
            assert res[i + 1][0].tobytes() == res[1][0].tobytes() and res[i + 1][1].tobytes() == res[1][1].tobytes()
        compare_exact(*c.oracle(c.q, 5, 2, **WIDE), *res[2])
    finally:
        g.close()


# ---- the list-major kernel (ivfflat.hip k_ivfflat_lm) -------------------------------------------------------------------
# 33 queries x 4 probes = 132 pairs >= 2 nlist, d in {16, 32, 64, 96, 128}, no list mask: list-major.  Lists of about 190 rows:
# two 128-row chunks with a partial one; a popular list is probed by more than 32 queries: a second query tile with a partial.
@pytest.mark.parametrize("dtype,d,metric", [("float16", 16, L2), ("uint8", 16, IP), ("int8", 32, L2), ("float16", 32, IP),
                                            ("uint8", 64, L2), ("int8", 64, IP), ("float16", 96, L2), ("int8", 96, IP),
                                            ("uint8", 128, L2), ("float16", 128, IP), ("int8", 128, L2)])
def test_list_major_kernel_over_narrow_rows(dtype, d, metric):
    c = R.Case(d, dtype, metric, seed=d)
    if dtype == "float16":
        assert (c.W != c.base).any()
    p = Pair(c)
    try:
        p.check(c.q, 10, 4)
        p.check(c.q, 1, 16)      # every list probed by every query: two query tiles per list
        if d in (16, 128):
            p.check_filtered(c.q, 10, 4, seed=d)
    finally:
        p.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_list_major_kernel_with_an_empty_list_and_a_superseded_entry(dtype):
    """list 5 is empty and probed (tests/test_ivfflat_rows_cpu.py).  Then a vector moves to another list, as an Update moves
    it: its old entry stays with bit 63 set and must be skipped; its row is rewritten through raw_write and the search sees
    the new row."""
    c = R.Case(32, dtype, L2, empty=5, seed=3)
    p = Pair(c)
    try:
        p.check(c.q, 10, 4)
        src = max(range(c.nlist), key=lambda l: len(c.lists[l]))
        dst = (src + 1) % c.nlist if (src + 1) % c.nlist != 5 else (src + 2) % c.nlist
        vid = int(c.lists[src][3])
        new = c.W[int(c.lists[dst][0])].copy()      # a neighbour of a row of dst, one step away in one element ...
        new[1] += 1.0 if new[1] < 100 else -1.0
        new = R.widened(new[None], dtype)[0]        # ... and a value the store holds exactly
        c.o.update_code(dst, vid, np.zeros(1, np.uint8))
        c.raw[vid] = new
        p.both(lambda h: h.update(dst, vid, np.zeros(1, np.uint8)))
        p.both(lambda h: h.raw_write(vid, new[None]))
        ids = p.g.get_list(src)[0]
        assert (ids < 0).sum() == 1 and np.array_equal(ids, c.o.get_list(src)[0])
        q = np.concatenate([c.q, new[None] + 0.125])      # the last query's nearest row is the rewritten one
        D, I = p.check(q, 10, 4)
        assert I[-1, 0] == vid
        D, I = p.check(q[-2:], 10, 4)      # 8 pairs: the small path over the same state
        assert I[-1, 0] == vid
    finally:
        p.close()


# ---- the pair kernel (rerank.hip k_ivfflat_scan), chunked path ---------------------------------------------------------
# d = 20, 33, 100 have no list-major form: 40 queries x 4 probes go to one workgroup per pair.  d = 33: rows aligned to their
# element only; d = 20: byte rows aligned to 4 bytes, half rows to 8; d = 100: the short last chunk of rerank_dist8.
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [20, 33, 100])
def test_pair_kernel_over_narrow_rows(dtype, d):
    for metric in (L2, IP):
        c = R.Case(d, dtype, metric, nq=40, seed=d)
        p = Pair(c)
        try:
            p.check(c.q, 10, 4)
            if metric == L2:
                p.check_filtered(c.q, 10, 4, seed=d)
        finally:
            p.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_pair_kernel_at_d_128_below_the_list_major_threshold(dtype):
    """7 queries x 4 probes = 28 pairs < 2 nlist with the small path off: the chunked path's pair kernel at a d that has a
    list-major form (16-byte row loads)"""
    c = R.Case(128, dtype, L2, nq=7, seed=5)
    p = Pair(c, small_path=False)
    try:
        p.check(c.q, 10, 4)
        p.check(c.q[:1], 100, 4)
    finally:
        p.close()


# ---- the small path (ivfflat_small) -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,d,metric", [("float16", 128, L2), ("uint8", 33, IP), ("int8", 64, L2), ("float16", 20, IP)])
def test_small_path_over_narrow_rows(dtype, d, metric):
    """1 and 7 queries x 4 probes: fewer pairs than 2 nlist, small path on (the default)"""
    c = R.Case(d, dtype, metric, nq=7, seed=6)
    p = Pair(c, small_path=True)
    try:
        for nq in (1, 7):
            p.check(c.q[:nq], 10, 4)
            p.check(c.q[:nq], 300, 4)
    finally:
        p.close()


# ---- exact ties -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nq", [33, 7], ids=["list_major", "small_path"])
def test_ties_at_the_k_cut_over_narrow_rows(dtype, nq):
    """every row occurs four times, so ranks 8 .. 11 hold one distance and k = 10 cuts the group (shown with the oracle in
    tests/test_ivfflat_rows_cpu.py): with exact ties on the survivors are the reference heap's, with them off the device's own --
    and the fp32 store's either way"""
    for metric in (L2, IP):
        c = R.Case(64, dtype, metric, ties=True, seed=7)
        p = Pair(c)
        try:
            p.check(c.q[:nq], R.TIE_K, 4, exact_ties=1)
            p.check(c.q[:nq], R.TIE_K, 4, exact_ties=-1)
            if nq == 7:
                p.both(lambda h: h.set_small_path(False))      # the chunked path's tie replay, pair kernel
                p.check(c.q[:nq], R.TIE_K, 4, exact_ties=1)
        finally:
            p.close()
