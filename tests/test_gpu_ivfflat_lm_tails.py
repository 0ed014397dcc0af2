"""GPU: the list-major IVFFLAT scan of row lengths that are no multiple of 16 (ivfflat.hip k_ivfflat_lmt behind
gamma_hip_set_ivfflat_lm_tails).

Every case holds the same lists and rows in two handles -- `on` with the switch on, `off` with it off, which is the pair kernel and
nothing else different -- and, for a narrow store, in a third: an fp32 store of the widened rows with the switch on.  It checks
  * `on` against the CPU oracle's IVFFLAT search, labels and distance bits at every rank (compare_exact, exact ties on);
  * byte equality of D and I across the handles;
  * the counters: `on` (and the fp32 store) counted tail chunks and nothing in ivfflat_scan_stats, `off` pair chunks only.
Base shape: tests/ivfflat_lm_data.py's -- nlist 16, N = 3001, 33 queries x 4 probes (132 pairs >= 2 nlist), k = 10."""
import itertools

import numpy as np
import pytest

from gamma_amd import api, plugin
from oracle import binding as B
from tests import ivfflat_lm_data as LM
from tests.parity import compare_exact

pytestmark = pytest.mark.gpu

WIDE = dict(min_score=-3e38, max_score=3e38)
L2, IP = B.METRIC_L2, B.METRIC_IP
PAIR, SLICED = 1, 3      # ivfflat_scan_stats


class Handles:
    def __init__(self, case, dtype=None, tails=(True, False)):
        """dtype: the store's element type, the case's by default ("float32": fp32 stores of the case's widened rows)"""
        self.c = case
        dtype = dtype or case.dtype
        rows = case.base if dtype == case.dtype else case.W
        self.all = [self._handle(dtype, rows, t) for t in tails]      # on, off
        if dtype != "float32":
            self.all.append(self._handle("float32", case.W, True))
        self.tails = [g.get_ivfflat_lm_tails() for g in self.all]

    def _handle(self, dtype, rows, tails):
        c = self.c
        g = api.GammaHip(0)
        g.ivfflat_init(c.d, c.nlist, c.metric)
        g.ivfflat_set_trained(c.cc)
        c.load(g)
        g.raw_init(c.d, dtype)
        g.raw_append(rows)
        if dtype != "float32":
            g.set_ivfflat_narrow_rows(True)
        g.set_ivfflat_lm_tails(tails)
        return g

    def close(self):
        for g in self.all:
            g.close()

    def each(self, f):
        for g in self.all:
            f(g)

    def check(self, q, k, P, win=WIDE, bm=None, docs=None, other=PAIR):
        """other: what a handle with the switch off -- or a length the switch does not concern -- counts"""
        ctx_kw, kw = {}, {}
        if bm is not None:
            ctx_kw["docids_bitmap"] = bm
        if docs is not None:
            ctx_kw["range_filters"] = [B.make_range_filter(docs)]
            kw["range_filters"] = [api.make_range_filter(docs)]
        D, I = self.c.oracle(q, k, P, **win, **ctx_kw)
        args = api.SearchArgs(metric=self.c.metric, nprobe=P, exact_ties=1, **win, **kw)
        res = [g.ivfflat_search(q, k, args) for g in self.all]
        compare_exact(D, I, *res[0])
        for Dg, Ig in res[1:]:
            assert Dg.tobytes() == res[0][0].tobytes() and Ig.tobytes() == res[0][1].tobytes()
        for g, on in zip(self.all, self.tails):
            t, s = g.ivfflat_lm_tail_stats(reset=True), g.ivfflat_scan_stats(reset=True)
            if on and other == PAIR:
                assert t > 0 and not any(s), (t, s)
            else:
                assert t == 0 and s[other] > 0 and all(s[i] == 0 for i in range(4) if i != other), (t, s)
        return D, I


def tile_queries(c, qtile):
    """40 queries around three centroids (LM.many_queries_case at this case's length): a list probed by more than qtile queries and
    one by exactly qtile, from the oracle's assignment"""
    noise = 0.01 * np.random.default_rng(411).standard_normal((40, c.d)).astype(np.float32)
    groups = np.repeat([0, 1, 2], [qtile + 1, qtile, 40 - 2 * qtile - 1])
    for abe in itertools.permutations(range(c.nlist), 3):
        q = np.ascontiguousarray(c.cc[np.array(abe)[groups]] + noise)
        cnt = LM.probes_per_list(c, q, LM.MANY_P)
        if (cnt > qtile).any() and (cnt == qtile).any():
            return q
    raise AssertionError("no triple of centroids gives the per-list counts the case needs")


def run_filtered(h, c):
    """delete bitmap + range filter, then a score window on top"""
    rng = np.random.default_rng(21)
    dead = rng.choice(c.N, c.N // 7, replace=False)
    bm = np.zeros((c.N >> 3) + 1, dtype=np.uint8)
    np.bitwise_or.at(bm, dead >> 3, (1 << (dead & 7)).astype(np.uint8))
    docs = rng.choice(c.N, 3 * c.N // 4, replace=False)
    h.each(lambda g: g.bitmap_upload(bm, c.N))
    Dw, Iw = h.check(c.q, 10, 4, bm=bm, docs=docs)
    fin = Dw[Iw >= 0]
    win = dict(min_score=float(np.quantile(fin, 0.2)), max_score=float(np.quantile(fin, 0.9)))
    D, _ = h.check(c.q, 10, 4, win=win, bm=bm, docs=docs)
    assert D.tobytes() != Dw.tobytes()      # the window cut something


def run_edge(h, c):
    """lists of 128 and 129 rows and an empty probed one; then a vector moves to another list, as an Update moves it: its old
    entry stays with bit 63 set and must be skipped, and the search sees the rewritten row"""
    assert [len(c.lists[l]) for l in (LM.EDGE_128, LM.EDGE_129, LM.EDGE_EMPTY)] == [128, 129, 0]
    cnt = LM.probes_per_list(c, c.q, 4)
    assert cnt[LM.EDGE_128] > 0 and cnt[LM.EDGE_129] > 0 and cnt[LM.EDGE_EMPTY] > 0
    h.check(c.q, 10, 4)
    vid = int(c.lists[LM.EDGE_128][3])
    new = c.W[int(c.lists[LM.EDGE_129][0])].copy()
    new[1] += 1.0
    c.o.update_code(LM.EDGE_129, vid, np.zeros(1, np.uint8))
    c.raw[vid] = new
    h.each(lambda g: g.update(LM.EDGE_129, vid, np.zeros(1, np.uint8)))
    h.each(lambda g: g.raw_write(vid, new[None]))
    ids = h.all[0].get_list(LM.EDGE_128)[0]
    assert len(ids) == 128 and (ids < 0).sum() == 1
    D, I = h.check(np.concatenate([c.q, new[None] + 0.125]), 10, 4)
    assert I[-1, 0] == vid


def plain(dtype, metric, ds):
    return [(dtype, metric, d, "plain") for d in ds]


CASES = (
    # fp32, 16-byte loads: no piece + the 4-lane step | 8-step + 4 | 16 + 4 | 16 + 8 | 16 + 8 + 4 | 64 + 32, r = 4 | two slabs + 32, r = 12
    plain("float32", L2, [4, 12, 20, 24, 28, 100, 300]) + plain("float32", IP, [4, 12, 20, 24, 28, 100, 300])
    # 8-byte loads | 4-byte loads: the masked step at 1..3 lanes with and without each earlier step | ... across a slab boundary
    + plain("float32", L2, [18, 22]) + plain("float32", L2, [1, 3, 7, 15, 17, 19, 21, 23, 27, 29, 31]) + plain("float32", L2, [133, 141])
    # narrow rows: float16 by 16 / 8 / 4 / 2 bytes, bytes by 8 / 4 / 2 / 1
    + [(t, L2, d, "plain") for t in ("float16", "uint8", "int8") for d in (24, 20, 18, 17)]
    + [(t, IP, 100, "plain") for t in ("float16", "uint8", "int8")]
    + [("float32", L2, 21, "filtered"), ("float32", L2, 21, "edge"), ("uint8", L2, 21, "ties"), ("float32", L2, 20, "tiles"),
       ("float32", L2, 144, "sliced")])


@pytest.mark.parametrize("dtype,metric,d,mode", CASES, ids=lambda v: {L2: "l2", IP: "ip"}.get(v, str(v)))
def test_tail_kernel(dtype, metric, d, mode):
    esz = {"float32": 4, "float16": 2}.get(dtype, 1)
    kind, load, qtile = api.ivfflat_lm_tail_shape(d, esz)
    assert kind == (0 if mode == "sliced" else 3) and api.ivfflat_lm_shape(d)[0] == (2 if mode == "sliced" else 0)
    if mode == "edge":
        c = LM.Case(d, dtype, metric, empty=LM.EDGE_EMPTY, seed=19, sizes={LM.EDGE_128: 128, LM.EDGE_129: 129})
    else:
        c = LM.Case(d, dtype, metric, seed=d, ties=mode == "ties")
    h = Handles(c, dtype="float32" if mode == "ties" else None, tails=(True,) if mode == "sliced" else (True, False))
    try:
        if mode == "plain":
            h.check(c.q, 10, 4)
        elif mode == "filtered":
            run_filtered(h, c)
        elif mode == "edge":
            run_edge(h, c)
        elif mode == "ties":      # integer-valued rows, every distinct row four times: the replay agrees at every rank
            D, I = c.oracle(c.q, LM.TIE_K, 4, **WIDE)
            assert ((D[:, 1:] == D[:, :-1]) & (I[:, 1:] != I[:, :-1])).any(axis=1).all()
            h.check(c.q, LM.TIE_K, 4)
        elif mode == "tiles":      # a full tile plus a partial one on one list, exactly one full tile on another
            q = tile_queries(c, qtile)
            cnt = LM.probes_per_list(c, q, LM.MANY_P)
            assert len(q) == 40 and (cnt >= 17).any() and (cnt == qtile).any(), cnt
            h.check(q, 10, LM.MANY_P)
        else:      # a multiple of 16 with the switch on: the row-sliced kernel, as before
            h.check(c.q, 10, 4, other=SLICED)
    finally:
        h.close()


def test_plugin_model_with_lm_tails():
    """HIPIVFFLAT with "lm_tails": 1 at d = 100 answers 33 queries as the model without the key does, byte for byte, and its tail
    counter moves; any other value fails Init"""
    c = LM.Case(100, "float32", L2, seed=100)
    res = []
    for extra in (', "lm_tails": 1', ""):
        m = plugin.PluginModel("HIPIVFFLAT", c.d, '{"ncentroids": %d, "nprobe": 4, "metric_type": "L2"%s}' % (c.nlist, extra),
                               indexing_size=1500)
        try:
            m.store(c.W)
            assert m.set_trained(c.cc, np.zeros((256, c.d), np.float32)) == 0
            assert m.add(c.W)
            res.append(m.search(c.q, 10, "") + (m.ivfflat_lm_tail_chunks(),))
        finally:
            m.close()
    assert res[0][0].tobytes() == res[1][0].tobytes() and res[0][1].tobytes() == res[1][1].tobytes()
    assert (res[0][1][:, 0] >= 0).all() and res[0][2] > 0 and res[1][2] == 0
    with pytest.raises(api.GammaHipError):
        plugin.PluginModel("HIPIVFFLAT", c.d, '{"ncentroids": 16, "metric_type": "L2", "lm_tails": 2}')
