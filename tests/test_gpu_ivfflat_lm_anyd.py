"""GPU: the row-sliced list-major IVFFLAT scan (ivfflat.hip k_ivfflat_lms): every row length that is a
multiple of 16 up to 4096 and not one of {16, 32, 64, 96, 128}.

Every case checks three things:
  * the CPU oracle's IVFFLAT search over the same lists and rows, labels and distance bits at every rank (compare_exact, exact
    ties on, no query left out);
  * byte equality of D and I with a second handle that holds the same lists and rows and has a list mask that owns EVERY list,
    which sends it to the pair kernel (one workgroup per (query, probe) pair) with nothing else changed;
  * through ivfflat_scan_stats, that the first handle counted a chunk of the sliced kernel and none of the pair kernel, and the
    second the reverse.
Base shape: nlist 16, N = 3001 (lists of about 190 rows: one full 128-row chunk and a partial one), 33 queries x 4 probes (132
pairs >= 2 nlist: list-major), k = 10.  The data is tests/ivfflat_lm_data.py's, examined on the CPU by tests/test_ivfflat_lm_cpu.py."""
import numpy as np
import pytest

from gamma_amd import api
from oracle import binding as B
from tests import ivfflat_lm_data as LM
from tests import ivfflat_rows_data as R
from tests.parity import compare_exact

pytestmark = pytest.mark.gpu

WIDE = dict(min_score=-3e38, max_score=3e38)
L2, IP = B.METRIC_L2, B.METRIC_IP
SMALL, PAIR, FIXED, SLICED = 0, 1, 2, 3      # ivfflat_scan_stats


def bitmap_of(n, dead):
    bm = np.zeros((n >> 3) + 1, dtype=np.uint8)
    np.bitwise_or.at(bm, dead >> 3, (1 << (dead & 7)).astype(np.uint8))
    return bm


class Handles:
    """lm: the store under test behind the lists of the case; pair: the same with a list mask owning every list (the pair
    kernel); f32 (narrow stores only): the fp32 store of the widened rows, list-major"""

    def __init__(self, case, lm_stat=SLICED, dtype=None):
        """dtype: the store's element type, the case's by default ("float32": fp32 stores of the case's widened rows)"""
        self.c, self.lm_stat = case, lm_stat
        dtype = dtype or case.dtype
        rows = case.base if dtype == case.dtype else case.W
        self.lm = self._handle(dtype, rows)
        self.pair = self._handle(dtype, rows)
        self.pair.set_list_mask(np.ones(case.nlist, np.uint8))
        self.all = [self.lm, self.pair]
        if dtype != "float32":
            self.all.append(self._handle("float32", case.W))
            assert self.lm.raw_elem_type() == 1 + R.DTYPES.index(dtype) and self.all[2].raw_elem_type() == 0

    def _handle(self, dtype, rows):
        c = self.c
        g = api.GammaHip(0)
        g.ivfflat_init(c.d, c.nlist, c.metric)
        g.ivfflat_set_trained(c.cc)
        c.load(g)
        g.raw_init(c.d, dtype)
        g.raw_append(rows)
        if dtype != "float32":
            g.set_ivfflat_narrow_rows(True)
        return g

    def close(self):
        for g in self.all:
            g.close()

    def each(self, f):
        for g in self.all:
            f(g)

    def check(self, q, k, P, win=WIDE, bm=None, docs=None):
        ctx_kw, kw = {}, {}
        if bm is not None:
            ctx_kw["docids_bitmap"] = bm
        if docs is not None:
            ctx_kw["range_filters"] = [B.make_range_filter(docs)]
            kw["range_filters"] = [api.make_range_filter(docs)]
        D, I = self.c.oracle(q, k, P, **win, **ctx_kw)
        args = api.SearchArgs(metric=self.c.metric, nprobe=P, exact_ties=1, **win, **kw)
        self.each(lambda g: g.ivfflat_scan_stats(reset=True))
        res = [g.ivfflat_search(q, k, args) for g in self.all]
        compare_exact(D, I, *res[0])
        for Dg, Ig in res[1:]:
            assert Dg.tobytes() == res[0][0].tobytes() and Ig.tobytes() == res[0][1].tobytes()
        # which kernel scanned: the handle under test list-major and never per pair, the masked one the reverse
        for g in self.all:
            s = g.ivfflat_scan_stats()
            ran = PAIR if g is self.pair else self.lm_stat
            assert s[ran] > 0 and all(s[i] == 0 for i in range(4) if i != ran), (ran, s)
        return D, I

    def check_filtered(self, q, k, P, seed):
        """delete bitmap + range filter + score window"""
        N = self.c.N
        rng = np.random.default_rng(seed)
        bm = bitmap_of(N, rng.choice(N, N // 7, replace=False))
        docs = rng.choice(N, 3 * N // 4, replace=False)
        self.each(lambda g: g.bitmap_upload(bm, N))
        Dw, Iw = self.check(q, k, P, bm=bm, docs=docs)
        fin = Dw[Iw >= 0]
        win = dict(min_score=float(np.quantile(fin, 0.2)), max_score=float(np.quantile(fin, 0.9)))
        D, I = self.check(q, k, P, win=win, bm=bm, docs=docs)
        assert D.tobytes() != Dw.tobytes()      # the window cut something


def shape_of(d):
    kind, slab, qtile = api.ivfflat_lm_shape(d)
    assert kind == 2 and slab > 0 and qtile > 0
    return slab, qtile


# ---- slab boundaries, fp32 rows -----------------------------------------------------------------------------------------
# one partial slab | a full slab + 16 | two full slabs | two full + 16 | six slabs
@pytest.mark.parametrize("metric", [L2, IP], ids=["l2", "ip"])
@pytest.mark.parametrize("d", [48, 144, 256, 272, 768])
def test_sliced_kernel_over_fp32_rows(d, metric):
    shape_of(d)
    c = LM.Case(d, "float32", metric, seed=d)
    h = Handles(c)
    try:
        h.check(c.q, 10, 4)
        if d == 144:
            h.check(c.q, 1, 16)      # every list probed by every query: 33 queries = two full tiles and a tile of one
    finally:
        h.close()


# ---- narrow rows: widened on load, slab by slab ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("d,metric", [(144, L2), (768, IP)])
def test_sliced_kernel_over_narrow_rows(dtype, d, metric):
    """the narrow store list-major, the narrow store per pair and the fp32 store of the widened rows: the same bytes"""
    c = LM.Case(d, dtype, metric, seed=d + 1)
    if dtype == "float16":
        assert (c.W != c.base).any()
    h = Handles(c)
    try:
        h.check(c.q, 10, 4)
    finally:
        h.close()


# ---- query tiles ---------------------------------------------------------------------------------------------------------
def test_more_queries_on_a_list_than_one_tile():
    """40 queries around three centroids: a list probed by more than qtile queries (a second, partial tile) and one probed by
    exactly qtile (one full tile, no second) -- asserted from the oracle's coarse assignment before the GPU call"""
    _, qtile = shape_of(144)
    c, q = LM.many_queries_case(qtile)
    cnt = LM.probes_per_list(c, q, LM.MANY_P)
    assert len(q) == 40 and (cnt > qtile).any() and (cnt == qtile).any(), cnt
    h = Handles(c)
    try:
        h.check(q, 10, LM.MANY_P)
    finally:
        h.close()


# ---- edge lists ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "int8"])
def test_lists_of_128_and_129_rows_an_empty_list_and_a_superseded_entry(dtype):
    """then a vector moves to another list, as an Update moves it: its old entry stays with bit 63 set and must be skipped; its
    row is rewritten and the search sees the new row"""
    c = LM.edge_case(dtype)
    assert [len(c.lists[l]) for l in (LM.EDGE_128, LM.EDGE_129, LM.EDGE_EMPTY)] == [128, 129, 0]
    cnt = LM.probes_per_list(c, c.q, 4)
    assert cnt[LM.EDGE_128] > 0 and cnt[LM.EDGE_129] > 0 and cnt[LM.EDGE_EMPTY] > 0
    h = Handles(c)
    try:
        h.check(c.q, 10, 4)
        src, dst = LM.EDGE_128, LM.EDGE_129      # the full chunk keeps 128 entries, one of them dead; the other grows to 130
        vid = int(c.lists[src][3])
        new = c.W[int(c.lists[dst][0])].copy()
        new[1] += 1.0 if new[1] < 100 else -1.0
        if dtype != "float32":
            new = R.widened(new[None], dtype)[0]
        c.o.update_code(dst, vid, np.zeros(1, np.uint8))
        c.raw[vid] = new
        h.each(lambda g: g.update(dst, vid, np.zeros(1, np.uint8)))
        h.each(lambda g: g.raw_write(vid, new[None]))
        ids = h.lm.get_list(src)[0]
        assert len(ids) == 128 and (ids < 0).sum() == 1 and np.array_equal(ids, c.o.get_list(src)[0])
        q = np.concatenate([c.q, new[None] + 0.125])      # the last query's nearest row is the rewritten one
        D, I = h.check(q, 10, 4)
        assert I[-1, 0] == vid
    finally:
        h.close()


# ---- filters ---------------------------------------------------------------------------------------------------------------
def test_delete_bitmap_range_filter_and_score_window():
    c = LM.Case(272, "float32", L2, seed=15)
    h = Handles(c)
    try:
        h.check_filtered(c.q, 10, 4, seed=272)
    finally:
        h.close()


# ---- exact ties ------------------------------------------------------------------------------------------------------------
def test_exact_ties_over_integer_valued_rows():
    """every distinct row four times: the replay has to agree with the oracle at every rank of every query"""
    c = LM.tie_case()
    D, I = c.oracle(c.q, LM.TIE_K, 4, **WIDE)
    assert ((D[:, 1:] == D[:, :-1]) & (I[:, 1:] != I[:, :-1])).any(axis=1).all()
    h = Handles(c, dtype="float32")      # fp32 stores of the (integer-valued) rows
    try:
        h.check(c.q, LM.TIE_K, 4)
    finally:
        h.close()


# ---- the grid-stride walk --------------------------------------------------------------------------------------------------
def test_more_work_units_than_persistent_workgroups():
    c = LM.grid_case()
    _, qtile = shape_of(c.d)
    assert LM.work_units(c, c.q, LM.GRID_P, qtile) > 2048      # (the launch has 2048 workgroups: u += gridDim.x is walked)
    h = Handles(c)
    try:
        h.check(c.q, 10, LM.GRID_P)
    finally:
        h.close()


# ---- the other two kernels are where they were ------------------------------------------------------------------------------
def test_fixed_lengths_keep_the_fixed_kernel_and_other_lengths_the_pair_kernel():
    assert api.ivfflat_lm_shape(128)[0] == 1 and api.ivfflat_lm_shape(100)[0] == 0
    c = LM.Case(128, "float32", L2, seed=16)
    h = Handles(c, lm_stat=FIXED)
    try:
        h.check(c.q, 10, 4)
    finally:
        h.close()
    c = LM.Case(100, "float32", L2, seed=17)
    h = Handles(c, lm_stat=PAIR)
    try:
        h.check(c.q, 10, 4)
    finally:
        h.close()
