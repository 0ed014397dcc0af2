"""GPU: the IVFFLAT list-shard building blocks (include/gamma_hip.h: gamma_hip_ivfflat_coarse_device / _search_shard / _merge /
_shard_export_rows / _shard_export / _merge_replay), W handles on device 0 driven from Python as shards
(tests/ivfflat_shard_emul.py).  Every case is compared with the CPU oracle's IVFFLAT search over the whole index (compare_exact:
distance bits and labels at every rank, no query left out) and, byte for byte, with ONE handle that holds every list.

Shapes: N about 3000, nlist 16, 33 queries; rows of 128 floats (the fixed list-major kernel), 144 (the row-sliced one) and 24
(the pair kernel), dense and sparse fp32 stores.  The data are tests/ivfflat_lm_data.py's and tests/ivfflat_shard_ref.py's,
examined on the CPU by tests/test_ivfflat_shard_cpu.py."""
import numpy as np
import pytest

from gamma_amd import api
from oracle import binding as B
from tests import ivfflat_lm_data as LM
from tests import ivfflat_shard_emul as EM
from tests import ivfflat_shard_ref as SR
from tests.parity import compare_exact, compare_topk

pytestmark = pytest.mark.gpu

L2, IP = B.METRIC_L2, B.METRIC_IP
WIDE = SR.WIDE
SMALL, PAIR, FIXED, SLICED = 0, 1, 2, 3      # ivfflat_scan_stats
LM_STAT = {128: FIXED, 144: SLICED, 24: PAIR}


def one_handle(c, lists=None):
    g = api.GammaHip(0)
    g.ivfflat_init(c.d, c.nlist, c.metric)
    g.ivfflat_set_trained(c.cc)
    lists = c.lists if lists is None else lists
    used = [l for l in range(c.nlist) if len(lists[l])]
    vids = np.concatenate([lists[l] for l in used])
    g.add_keys_batch(used, [len(lists[l]) for l in used], vids, np.zeros((len(vids), 1), np.uint8))
    g.raw_init(c.d, "float32")
    g.raw_append(c.raw)
    return g


class Rig:
    def __init__(self, c, W, owner, sparse):
        self.c, self.W = c, W
        self.shards = EM.make_shards(c, owner, W, sparse)
        self.one = one_handle(c)
        self.all = self.shards + [self.one]

    def close(self):
        for g in self.all:
            g.close()

    def check(self, q, k, P, win=WIDE, bm=None, docs=None, exact_ties=1, **emul_kw):
        ctx_kw, kw = {}, {}
        if bm is not None:
            ctx_kw["docids_bitmap"] = bm
        if docs is not None:
            ctx_kw["range_filters"] = [B.make_range_filter(docs)]
            kw["range_filters"] = [api.make_range_filter(docs)]
        D0, I0 = self.c.oracle(q, k, P, **win, **ctx_kw)
        args = api.SearchArgs(metric=self.c.metric, nprobe=P, exact_ties=exact_ties, **win, **kw)
        for g in self.shards:
            g.ivfflat_scan_stats(reset=True)
        D, I, nf = EM.sharded_search(self.shards, q, k, args, **emul_kw)
        D1, I1 = self.one.ivfflat_search(q, k, args)
        if exact_ties > 0:
            compare_exact(D0, I0, D, I)
            pad = I1 == -1
            assert np.array_equal(I, I1) and D[~pad].tobytes() == D1[~pad].tobytes()
        else:      # distances identical at every rank; ids may differ inside groups of equal distances only
            compare_topk(D1, I1, D, I)
        return D, I, nf


@pytest.fixture(scope="module")
def cases():
    return {}


def case_of(cases, d, metric):
    key = (d, metric)
    if key not in cases:
        cases[key] = LM.Case(d, "float32", metric, seed=60 + d)
    return cases[key]


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("d,metric,W", [(128, L2, 2), (144, IP, 3), (24, L2, 4), (144, L2, 4), (128, IP, 3)])
def test_shards_equal_one_handle_and_the_oracle(cases, d, metric, W, sparse):
    c = case_of(cases, d, metric)
    r = Rig(c, W, SR.owners_mod(c.nlist, W), sparse)
    try:
        r.check(c.q, 10, 4)
        # 33 x 4 pairs >= 2 nlist: every shard scanned list-major under its mask (d 24 has no list-major form)
        for g in r.shards:
            s = g.ivfflat_scan_stats()
            assert s[LM_STAT[d]] > 0 and all(s[i] == 0 for i in range(4) if i != LM_STAT[d]), s
        # 7 x 4 pairs < 2 nlist: the pair kernel
        r.check(c.q[:7], 10, 4)
        for g in r.shards:
            s = g.ivfflat_scan_stats()
            assert s[PAIR] > 0 and s[FIXED] == 0 and s[SLICED] == 0, s
        # k larger than the number of candidates (two probes of ~190 rows)
        D, I, _ = r.check(c.q, 500, 2)
        assert (I == -1).any()
    finally:
        r.close()


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
def test_a_shard_without_probed_lists_and_an_empty_sparse_store(sparse):
    """edge_case: a list of exactly 128 rows, one of 129, an empty one that queries probe.  Shard 1 owns ONE list (most queries
    probe none of its lists); shard 2 owns only the empty list: its sparse store never took a row"""
    c = LM.edge_case()
    assert [len(c.lists[l]) for l in (LM.EDGE_128, LM.EDGE_129, LM.EDGE_EMPTY)] == [128, 129, 0]
    cnt = LM.probes_per_list(c, c.q, 4)
    assert cnt[LM.EDGE_128] > 0 and cnt[LM.EDGE_129] > 0 and cnt[LM.EDGE_EMPTY] > 0 and cnt[LM.EDGE_129] < len(c.q)
    owner = np.zeros(c.nlist, dtype=np.int64)
    owner[LM.EDGE_129] = 1
    owner[LM.EDGE_EMPTY] = 2
    r = Rig(c, 3, owner, sparse)
    try:
        if sparse:
            assert r.shards[2].raw_count() == 0
        r.check(c.q, 10, 4)
    finally:
        r.close()


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
def test_an_entry_superseded_by_an_update(sparse):
    """a vector moves to another list of the same shard, as an Update moves it: its old entry keeps bit 63 and is skipped by
    the scan and the export; its row is rewritten (in place in the sparse store)"""
    c = LM.edge_case(seed=21)
    src, dst = LM.EDGE_128, LM.EDGE_129
    owner = SR.owners_mod(c.nlist, 2)
    owner[dst] = owner[src]
    r = Rig(c, 2, owner, sparse)
    try:
        vid = int(c.lists[src][3])
        new = c.W[int(c.lists[dst][0])].copy()
        new[1] += 1.0
        c.o.update_code(dst, vid, np.zeros(1, np.uint8))
        c.raw[vid] = new
        for g in (r.shards[owner[src]], r.one):
            g.update(dst, vid, np.zeros(1, np.uint8))
        if sparse:
            r.shards[owner[src]].raw_put([vid], new[None])
            r.one.raw_write(vid, new[None])
        else:
            for g in r.all:
                g.raw_write(vid, new[None])
        q = np.concatenate([c.q, new[None] + 0.125])
        D, I, _ = r.check(q, 10, 4)
        assert I[-1, 0] == vid
    finally:
        r.close()


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
def test_range_filter_deleted_docs_and_score_window(sparse):
    c = LM.Case(144, "float32", L2, seed=71)
    r = Rig(c, 3, SR.owners_by_size(c.lists, 3), sparse)
    try:
        N = c.N
        rng = np.random.default_rng(5)
        dead = rng.choice(N, N // 7, replace=False)
        bm = np.zeros((N >> 3) + 1, dtype=np.uint8)
        np.bitwise_or.at(bm, dead >> 3, (1 << (dead & 7)).astype(np.uint8))
        docs = rng.choice(N, 3 * N // 4, replace=False)
        for g in r.all:
            g.bitmap_upload(bm, N)
        Dw, Iw, _ = r.check(c.q, 10, 4, bm=bm, docs=docs)
        fin = Dw[Iw >= 0]
        win = dict(min_score=float(np.quantile(fin, 0.2)), max_score=float(np.quantile(fin, 0.9)))
        D, I, _ = r.check(c.q, 10, 4, win=win, bm=bm, docs=docs)
        assert D.tobytes() != Dw.tobytes()
    finally:
        r.close()


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("metric,W", [(L2, 2), (IP, 3), (L2, 4)])
def test_exact_ties_across_shards(metric, W, sparse):
    """every distinct row four times, the copies spread over two lists: the flag rule and the replay decide every query"""
    c = SR.TieCase(metric=metric, seed=3)
    owner = SR.owners_mod(c.nlist, W)
    _, _, info = SR.sharded_search(c, c.q, 10, 4, W, owner)
    assert info["cross"].any() and info["shard_cut"].any()
    r = Rig(c, W, owner, sparse)
    try:
        _, _, nf = r.check(c.q, 10, 4)
        assert nf >= int(info["flagged"].sum()) > 0
        # without the shards' cut flags the merge assumes the worst: no fewer queries replayed, the same result
        _, _, nf2 = r.check(c.q, 10, 4, use_shard_flags=False)
        assert nf2 >= nf
        # exact ties off: the merged top-k, no replay
        _, _, nf0 = r.check(c.q, 10, 4, exact_ties=-1)
        assert nf0 == 0
    finally:
        r.close()


def test_a_workspace_budget_that_forces_several_chunks():
    """the cut flags of every chunk survive (the second flag is what makes the merge flag a query whose shard dropped a tie)"""
    c = SR.TieCase(metric=L2, seed=3)
    owner = SR.owners_mod(c.nlist, 2)
    r = Rig(c, 2, owner, True)
    try:
        _, _, nf_one = r.check(c.q, 10, 4)
        longest = max(len(l) for l in c.lists)
        for g in r.shards:
            g.set_dist_budget(5 * 4 * longest * 4)      # five queries' slab rows per chunk: 33 queries = 7 chunks
        _, _, nf = r.check(c.q, 10, 4)
        assert nf == nf_one
    finally:
        r.close()


def test_a_float16_store_is_refused_with_its_message():
    c = LM.Case(24, "float32", L2, seed=72)
    g = api.GammaHip(0)
    try:
        g.ivfflat_init(c.d, c.nlist, c.metric)
        g.ivfflat_set_trained(c.cc)
        c.load(g)
        g.raw_init(c.d, "float16")
        g.raw_append(c.raw)
        import torch
        x = torch.from_numpy(c.q).cuda()
        pr = torch.zeros((len(c.q), 4), dtype=torch.int32, device="cuda")
        Dd = torch.zeros((len(c.q), 10), dtype=torch.float32, device="cuda")
        Id = torch.zeros((len(c.q), 10), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        args = api.SearchArgs(metric=c.metric, nprobe=4, **WIDE)
        with pytest.raises(api.GammaHipError, match="float16 raw store"):
            g.ivfflat_search_shard(x.data_ptr(), len(c.q), 0, pr.data_ptr(), 10, args, Dd.data_ptr(), Id.data_ptr())
        # limits are the single-handle search's: beyond them an error, never silence
        with pytest.raises(api.GammaHipError):
            g.ivfflat_search_shard(x.data_ptr(), len(c.q), 0, pr.data_ptr(), 5000, args, Dd.data_ptr(), Id.data_ptr())
        # the existing entry keeps its refusal of a sparse store
        s = EM.make_shards(c, np.zeros(c.nlist, dtype=np.int64), 1, True)[0]
        try:
            with pytest.raises(api.GammaHipError, match="this shard's rows only"):
                s.ivfflat_search(c.q, 10, args)
        finally:
            s.close()
    finally:
        g.close()
