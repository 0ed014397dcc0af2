"""W IVFFLAT list shards on ONE GPU driven through the C ABI from Python (tests/test_gpu_ivfflat_shard.py): the steps
gamma_hip_group_ivfflat_search runs, with the exchanges done by tensor indexing -- coarse quantizer on one handle, the shard
search on each, the merge and the tie phase on the owner of a query slice.  Several handles = several streams, and torch's own:
everything torch fills is complete (torch.cuda.synchronize) before a handle's kernels are enqueued on it, and every handle call
is synchronised before torch or another handle reads its output (tests/shard_emul.py)."""
import numpy as np
import torch

from gamma_amd import api


def make_shards(c, owner, W, sparse, lists=None):
    """one handle per owner over the case's lists: a list mask, the lists it owns, and the rows -- every row by vector id in a
    dense store, or the rows of ITS lists' vectors in a sparse one (raw_put).  A shard that owns no vector has an empty
    sparse store."""
    lists = c.lists if lists is None else lists
    out = []
    for w in range(W):
        g = api.GammaHip(0)
        g.ivfflat_init(c.d, c.nlist, c.metric)
        g.ivfflat_set_trained(c.cc)
        g.set_list_mask((np.asarray(owner) == w).astype(np.uint8))
        used = [l for l in range(c.nlist) if owner[l] == w and len(lists[l])]
        if used:
            vids = np.concatenate([lists[l] for l in used])
            g.add_keys_batch(used, [len(lists[l]) for l in used], vids, np.zeros((len(vids), 1), np.uint8))
        g.raw_init(c.d, "float32")
        if sparse:
            vids = np.concatenate([lists[l] for l in used]) if used else np.zeros(0, np.int64)
            g.raw_put(vids, c.raw[vids] if len(vids) else np.zeros((0, c.d), np.float32))
        else:
            g.raw_append(c.raw)
        out.append(g)
    return out


def sharded_search(shards, q, k, args, slices=None, use_shard_flags=True):
    """q: [nq, d] numpy.  slices: [(q0, q1, owner shard)] -- who merges which queries (default: two halves, shards 0 and W - 1).
    Returns (D, I, flagged) as numpy / int."""
    W = len(shards)
    dev = torch.device("cuda:0")
    x = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).to(dev)
    nq, d = x.shape
    P = args.p.nprobe
    if slices is None:
        h = (nq + 1) // 2
        slices = [(0, h, 0), (h, nq, W - 1)]
    cdis = torch.zeros((nq, P), dtype=torch.float32, device=dev)
    probe = torch.full((nq, P), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    shards[0].ivfflat_coarse_device(x.data_ptr(), nq, args, cdis.data_ptr(), probe.data_ptr())
    shards[0].synchronize()
    rd, ri, cf = [], [], []
    for g in shards:
        rdis = torch.zeros((nq, k), dtype=torch.float32, device=dev)
        rids = torch.full((nq, k), -7, dtype=torch.int64, device=dev)
        cut = torch.zeros((nq,), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        g.ivfflat_search_shard(x.data_ptr(), nq, cdis.data_ptr(), probe.data_ptr(), k, args, rdis.data_ptr(), rids.data_ptr())
        g.ivfpq_shard_cut_flags(nq, cut.data_ptr())
        g.synchronize()
        rd.append(rdis)
        ri.append(rids)
        cf.append(cut)
    D = torch.zeros((nq, k), dtype=torch.float32, device=dev)
    I = torch.full((nq, k), -7, dtype=torch.int64, device=dev)
    flagged = 0
    for q0, q1, r in slices:
        nql = q1 - q0
        if nql <= 0:
            continue
        own = shards[r]
        # the tables travel whole ([W][nq][k]); the merge takes its slice through q0 / nq_local
        all_dis = torch.stack(rd).contiguous()
        all_ids = torch.stack(ri).contiguous()
        cut_all = torch.stack(cf).contiguous()
        Dr = torch.zeros((nql, k), dtype=torch.float32, device=dev)
        Ir = torch.full((nql, k), -7, dtype=torch.int64, device=dev)
        xs = x[q0:q1].contiguous()
        prs = probe[q0:q1].contiguous()
        torch.cuda.synchronize()
        if use_shard_flags:
            own.ivfpq_merge_set_shard_flags(cut_all.data_ptr())
        own.ivfflat_merge(W, nq, k, args, all_dis.data_ptr(), all_ids.data_ptr(), q0, nql, Dr.data_ptr(), Ir.data_ptr())
        nf, d_list = own.ivfpq_merge_flagged()
        flagged += nf
        if nf:
            xf = torch.empty((nf, d), dtype=torch.float32, device=dev)
            pf = torch.empty((nf, P), dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            own.gather_rows(xs.data_ptr(), d, d_list, nf, xf.data_ptr())
            own.gather_rows(prs.data_ptr(), P, d_list, nf, pf.data_ptr())
            own.synchronize()
            stride = max(4, (max(g.ivfflat_shard_export_rows(nf, pf.data_ptr(), args) for g in shards) + 3) // 4 * 4)
            vals = torch.empty((W, nf, stride), dtype=torch.float32, device=dev)
            ids = torch.empty((W, nf, stride), dtype=torch.int64, device=dev)
            off = torch.empty((W, nf, P + 1), dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            for s, g in enumerate(shards):
                g.ivfflat_shard_export(nf, xf.data_ptr(), pf.data_ptr(), stride, args, vals[s].data_ptr(), ids[s].data_ptr(),
                                       off[s].data_ptr())
                g.synchronize()
            own.ivfflat_merge_replay(W, nf, xs.data_ptr(), stride, vals.data_ptr(), ids.data_ptr(), off.data_ptr(), k, args, d_list,
                                     Dr.data_ptr(), Ir.data_ptr())
        own.synchronize()
        D[q0:q1] = Dr
        I[q0:q1] = Ir
    torch.cuda.synchronize()
    return D.cpu().numpy(), I.cpu().numpy(), flagged
