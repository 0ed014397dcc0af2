"""GPU: the IVFFLAT list-shard entries over float16 / uint8 / int8 rows (gamma_hip_ivfflat_search_shard / _shard_export after
gamma_hip_set_ivfflat_narrow_rows), W handles on device 0 driven as shards by tests/ivfflat_shard_emul.py.

Every case is compared three ways, no query left out: with the CPU oracle's IVFFLAT search over the widened rows W
(compare_exact: distance bits and labels at every rank), byte for byte with ONE handle that holds every list and a dense store
of the same type, and byte for byte with shards that hold W as fp32 rows.  The inputs are tests/ivfflat_shard_rows_data.py's,
examined on the CPU by tests/test_ivfflat_shard_rows_cpu.py."""
import numpy as np
import pytest

from gamma_amd import api
from oracle import binding as B
from tests import ivfflat_lm_data as LM
from tests import ivfflat_shard_emul as EM
from tests import ivfflat_shard_ref as SR
from tests import ivfflat_shard_rows_data as RD
from tests.parity import compare_exact, compare_topk

pytestmark = pytest.mark.gpu

L2, IP = RD.L2, RD.IP
WIDE = SR.WIDE
K, P = RD.K, RD.P
SPARSE = pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
DTYPE = pytest.mark.parametrize("dtype", RD.DTYPES)


def make_shards(c, owner, W, sparse, dtype, ivfflat_switch=True):
    """EM.make_shards with a store of `dtype`: typed raw_init, the switches, then every row of the caller's `base` in a dense
    store or the rows of ITS lists' vectors in a sparse one.  dtype "float32": the widened rows W as fp32."""
    rows = c.W if dtype == "float32" else c.base
    out = []
    for w in range(W):
        g = api.GammaHip(0)
        g.ivfflat_init(c.d, c.nlist, c.metric)
        g.ivfflat_set_trained(c.cc)
        g.set_list_mask((np.asarray(owner) == w).astype(np.uint8))
        used = [l for l in range(c.nlist) if owner[l] == w and len(c.lists[l])]
        vids = np.concatenate([c.lists[l] for l in used]) if used else np.zeros(0, np.int64)
        if used:
            g.add_keys_batch(used, [len(c.lists[l]) for l in used], vids, np.zeros((len(vids), 1), np.uint8))
        g.raw_init(c.d, dtype)
        if dtype != "float32":
            if ivfflat_switch:
                g.set_ivfflat_narrow_rows(True)
            if sparse:
                g.set_sparse_narrow_rows(True)
        if sparse:
            g.raw_put(vids, rows[vids] if len(vids) else np.zeros((0, c.d), np.float32))
        else:
            g.raw_append(rows)
        out.append(g)
    return out


def one_handle(c, dtype):
    g = api.GammaHip(0)
    g.ivfflat_init(c.d, c.nlist, c.metric)
    g.ivfflat_set_trained(c.cc)
    c.load(g)
    g.raw_init(c.d, dtype)
    g.set_ivfflat_narrow_rows(True)
    g.raw_append(c.base)
    return g


class Rig:
    def __init__(self, c, W, owner, sparse, dtype):
        self.c, self.W, self.dtype = c, W, dtype
        self.all = []
        try:
            self.shards = make_shards(c, owner, W, sparse, dtype)
            self.all += self.shards
            self.wide = make_shards(c, owner, W, sparse, "float32")
            self.all += self.wide
            self.one = one_handle(c, dtype)
            self.all.append(self.one)
        except Exception:
            self.close()
            raise
        for g in self.shards:
            assert g.raw_elem_bytes() == R_ESZ[dtype]

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
        Dw, Iw, nfw = EM.sharded_search(self.wide, q, k, args, **emul_kw)
        D1, I1 = self.one.ivfflat_search(q, k, args)
        # the shards of the type against the shards holding W as fp32: the same bytes, ties or none, and the same flags
        assert D.tobytes() == Dw.tobytes() and I.tobytes() == Iw.tobytes() and nf == nfw
        if exact_ties > 0:
            compare_exact(D0, I0, D, I)
            pad = I1 == -1
            assert np.array_equal(I, I1) and D[~pad].tobytes() == D1[~pad].tobytes()
        else:      # distances identical at every rank; ids may differ inside groups of equal distances only
            compare_topk(D1, I1, D, I)
        return D, I, nf


R_ESZ = {"float16": 2, "uint8": 1, "int8": 1}


@SPARSE
@DTYPE
@pytest.mark.parametrize("d,metric,W", RD.SHAPES)
def test_shards_equal_the_oracle_one_handle_and_fp32_shards(d, metric, W, dtype, sparse):
    c = RD.case(d, dtype, metric)
    r = Rig(c, W, SR.owners_mod(c.nlist, W), sparse, dtype)
    try:
        r.check(c.q, K, P)
        # 33 x 4 pairs >= 2 nlist: every shard scanned list-major under its mask (d 24 and 20 have no list-major form)
        for g in r.shards:
            s = g.ivfflat_scan_stats()
            assert s[RD.LM_STAT[d]] > 0 and all(s[i] == 0 for i in range(4) if i != RD.LM_STAT[d]), s
        # 7 x 4 pairs < 2 nlist: the pair kernel
        r.check(c.q[:7], K, P)
        for g in r.shards:
            s = g.ivfflat_scan_stats()
            assert s[RD.PAIR] > 0 and s[RD.FIXED] == 0 and s[RD.SLICED] == 0, s
        # k larger than the number of candidates (two probes of ~190 rows)
        D, I, _ = r.check(c.q, 500, 2)
        assert (I == -1).any()
    finally:
        r.close()


@SPARSE
@DTYPE
def test_a_shard_without_probed_lists_and_an_empty_sparse_store(dtype, sparse):
    """lists of exactly 128 and 129 rows, an empty one that queries probe; shard 2 owns only the empty list: its sparse narrow
    store never took a row"""
    c = RD.edge_case(dtype)
    owner = np.zeros(c.nlist, dtype=np.int64)
    owner[LM.EDGE_129] = 1
    owner[LM.EDGE_EMPTY] = 2
    r = Rig(c, 3, owner, sparse, dtype)
    try:
        if sparse:
            assert r.shards[2].raw_count() == 0
        r.check(c.q, K, P)
    finally:
        r.close()


@SPARSE
@DTYPE
def test_an_entry_superseded_by_an_update(dtype, sparse):
    """a vector moves to another list of the same shard: its old entry keeps bit 63 and is skipped by the scan and the export;
    its row is rewritten -- in place, by raw_put, in the sparse store -- and converted by the store that takes it"""
    c = RD.edge_case(dtype, seed=RD.UPDATE_SEED)
    src, dst = LM.EDGE_128, LM.EDGE_129
    owner = SR.owners_mod(c.nlist, 2)
    owner[dst] = owner[src]
    r = Rig(c, 2, owner, sparse, dtype)
    try:
        vid = int(c.lists[src][3])
        new, held = RD.changed_row(c, dtype, int(c.lists[dst][0]))
        c.o.update_code(dst, vid, np.zeros(1, np.uint8))
        c.raw[vid] = held
        for g in (r.shards[owner[src]], r.wide[owner[src]], r.one):
            g.update(dst, vid, np.zeros(1, np.uint8))
        if sparse:
            live = r.shards[owner[src]].raw_sparse_stats()["live"]
            r.shards[owner[src]].raw_put([vid], new[None])
            assert r.shards[owner[src]].raw_sparse_stats()["live"] == live      # rewritten in place
            r.wide[owner[src]].raw_put([vid], held[None])
        else:
            for g in r.shards:
                g.raw_write(vid, new[None])
            for g in r.wide:
                g.raw_write(vid, held[None])
        r.one.raw_write(vid, new[None])
        q = np.concatenate([c.q, held[None] + 0.125])
        D, I, _ = r.check(q, K, P)
        assert I[-1, 0] == vid
    finally:
        r.close()


@SPARSE
@DTYPE
def test_range_filter_deleted_docs_and_score_window(dtype, sparse):
    c = RD.filter_case(dtype)
    r = Rig(c, 3, SR.owners_by_size(c.lists, 3), sparse, dtype)
    try:
        N = c.N
        rng = np.random.default_rng(5)
        dead = rng.choice(N, N // 7, replace=False)
        bm = np.zeros((N >> 3) + 1, dtype=np.uint8)
        np.bitwise_or.at(bm, dead >> 3, (1 << (dead & 7)).astype(np.uint8))
        docs = rng.choice(N, 3 * N // 4, replace=False)
        for g in r.all:
            g.bitmap_upload(bm, N)
        Dw, Iw, _ = r.check(c.q, K, P, bm=bm, docs=docs)
        fin = Dw[Iw >= 0]
        win = dict(min_score=float(np.quantile(fin, 0.2)), max_score=float(np.quantile(fin, 0.9)))
        D, I, _ = r.check(c.q, K, P, win=win, bm=bm, docs=docs)
        assert D.tobytes() != Dw.tobytes()
    finally:
        r.close()


@SPARSE
@DTYPE
@pytest.mark.parametrize("metric,W", RD.TIE_SHAPES)
def test_exact_ties_across_shards(metric, W, dtype, sparse):
    """every distinct row four times, the copies spread over two lists: the flag rule and the replay decide every query"""
    c = RD.tie_case(dtype, metric)
    owner = SR.owners_mod(c.nlist, W)
    _, _, info = SR.sharded_search(c, c.q, K, P, W, owner, **WIDE)
    assert info["cross"].any() and info["shard_cut"].any()
    r = Rig(c, W, owner, sparse, dtype)
    try:
        _, _, nf = r.check(c.q, K, P)
        assert nf >= int(info["flagged"].sum()) > 0
        # without the shards' cut flags the merge assumes the worst: no fewer queries replayed, the same result
        _, _, nf2 = r.check(c.q, K, P, use_shard_flags=False)
        assert nf2 >= nf
        # exact ties off: the merged top-k, no replay
        _, _, nf0 = r.check(c.q, K, P, exact_ties=-1)
        assert nf0 == 0
    finally:
        r.close()


@DTYPE
def test_a_workspace_budget_that_forces_several_chunks(dtype):
    c = RD.tie_case(dtype, L2)
    owner = SR.owners_mod(c.nlist, 2)
    r = Rig(c, 2, owner, True, dtype)
    try:
        _, _, nf_one = r.check(c.q, K, P)
        longest = max(len(l) for l in c.lists)
        for g in r.shards + r.wide:
            g.set_dist_budget(5 * 4 * longest * 4)      # five queries' slab rows per chunk: 33 queries = 7 chunks
        _, _, nf = r.check(c.q, K, P)
        assert nf == nf_one
    finally:
        r.close()


@DTYPE
def test_the_ivfflat_switch_off_still_refuses_with_the_stores_message(dtype):
    """the sparse narrow store exists (gamma_hip_set_sparse_narrow_rows), the IVFFLAT switch is off: every entry that reads rows
    refuses as before; switched on, the same handle answers; the single-handle search keeps its refusal of a sparse store"""
    import torch
    c = RD.case(24, dtype, IP)
    s = make_shards(c, np.zeros(c.nlist, dtype=np.int64), 1, True, dtype, ivfflat_switch=False)[0]
    try:
        nq = len(c.q)
        x = torch.from_numpy(c.q).cuda()
        pr = torch.zeros((nq, P), dtype=torch.int32, device="cuda")
        cd = torch.zeros((nq, P), dtype=torch.float32, device="cuda")
        Dd = torch.zeros((nq, K), dtype=torch.float32, device="cuda")
        Id = torch.zeros((nq, K), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        args = api.SearchArgs(metric=c.metric, nprobe=P, **WIDE)
        s.ivfflat_coarse_device(x.data_ptr(), nq, args, cd.data_ptr(), pr.data_ptr())      # reads no row: served
        s.synchronize()
        what = "float16 raw store" if dtype == "float16" else "8-bit raw store"
        with pytest.raises(api.GammaHipError, match=what):
            s.ivfflat_search_shard(x.data_ptr(), nq, cd.data_ptr(), pr.data_ptr(), K, args, Dd.data_ptr(), Id.data_ptr())
        s.set_ivfflat_narrow_rows(True)
        s.ivfflat_search_shard(x.data_ptr(), nq, cd.data_ptr(), pr.data_ptr(), K, args, Dd.data_ptr(), Id.data_ptr())
        s.synchronize()
        D0, I0 = c.oracle(c.q, K, P, **WIDE)
        compare_topk(D0, I0, Dd.cpu().numpy(), Id.cpu().numpy())
        with pytest.raises(api.GammaHipError, match="this shard's rows only"):
            s.ivfflat_search(c.q, K, args)
    finally:
        s.close()


def test_an_sq8_store_stays_refused_at_the_shard_entries():
    import torch
    c = RD.case(24, "uint8", IP)
    g = api.GammaHip(0)
    try:
        g.ivfflat_init(c.d, c.nlist, c.metric)
        g.ivfflat_set_trained(c.cc)
        c.load(g)
        g.raw_init(c.d, "sq8")
        g.raw_sq8_train(c.base)
        g.raw_append(c.base)
        g.set_ivfflat_narrow_rows(True)
        g.set_ivfflat_sq8_rows(True)
        nq = len(c.q)
        x = torch.from_numpy(c.q).cuda()
        pr = torch.zeros((nq, P), dtype=torch.int32, device="cuda")
        Dd = torch.zeros((nq, K), dtype=torch.float32, device="cuda")
        Id = torch.zeros((nq, K), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        args = api.SearchArgs(metric=c.metric, nprobe=P, **WIDE)
        with pytest.raises(api.GammaHipError, match="sq8 raw store"):
            g.ivfflat_search_shard(x.data_ptr(), nq, 0, pr.data_ptr(), K, args, Dd.data_ptr(), Id.data_ptr())
    finally:
        g.close()
