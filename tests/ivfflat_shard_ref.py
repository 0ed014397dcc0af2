"""The list-sharded IVFFLAT search restated in numpy on top of the CPU oracle (tests/test_ivfflat_shard_cpu.py; the GPU tests of
the shard entries and of the group use the same cases): a case's lists are split over W owners, every shard answers with the
oracle's IVFFLAT search over ITS lists, the owner merges the W x k candidates, flags the queries a tie can change and replays
their assembled streams through the IVFFLAT scanner's heap (go_heap_pop_push_stream: heap_pop + heap_push when dis < top, then
heap_reorder).  The result has to be B.ivfflat_search's on the whole index, labels at every rank.

The flag rule (include/gamma_hip.h, gamma_hip_ivfflat_merge) -- a query is replayed when
  (a) two of its k merged distances are equal, or
  (b) the merged cut passes through a group of equal distances: the shards' tables hold more entries equal to the merged k-th
      value than the merged table took, or
  (c) a shard table whose OWN cut went through a group of equal distances ends at the merged k-th value (the shard may have
      dropped members of that group).
rule="never" flags nothing: the test shows that the data then give a wrong answer, i.e. that they exercise the rule."""
import numpy as np

from oracle import binding as B
from tests import ivfflat_lm_data as LM

WIDE = dict(min_score=-3e38, max_score=3e38)


def owners_mod(nlist, W):
    return np.arange(nlist) % W


def owners_by_size(lists, W):
    """greedy longest-processing-time on the list lengths (gamma_hip_group_set_owners with weights)"""
    w = np.array([len(l) for l in lists], dtype=np.int64)
    order = sorted(range(len(lists)), key=lambda l: -w[l])      # (stable: ties keep the list order)
    load = np.zeros(W, dtype=np.int64)
    owner = np.zeros(len(lists), dtype=np.int64)
    for l in order:
        best = int(np.argmin(load))
        owner[l] = best
        load[best] += max(0, int(w[l])) + 1
    return owner


class TieCase(LM.Case):
    """integer-valued rows, every distinct row TIE_COPIES times -- and the copies of a row spread over TWO lists (every other
    copy goes to the row's second-nearest centroid), so that equal distances reach a query from lists of different owners"""

    def __init__(self, d=32, metric=B.METRIC_L2, N=3000, nlist=16, nq=33, seed=0):
        super().__init__(d, "uint8", metric, N=N, nlist=nlist, nq=nq, seed=seed, ties=True)
        W64, c64 = self.W.astype(np.float64), self.cc.astype(np.float64)
        dis = (W64 ** 2).sum(1)[:, None] - 2.0 * W64 @ c64.T + (c64 ** 2).sum(1)[None, :]
        near = np.argsort(dis, axis=1, kind="stable")[:, :2]
        seen = {}
        lno = np.empty(N, dtype=np.int64)
        for i in range(N):
            key = self.W[i].tobytes()
            n = seen.get(key, 0)
            seen[key] = n + 1
            lno[i] = near[i, n & 1]
        order = np.argsort(lno, kind="stable")
        self.lists = [order[lno[order] == l].astype(np.int64) for l in range(nlist)]
        self.o = B.OracleIVFPQ(d, nlist, 1, 8, metric)
        self.o.set_trained(self.cc, np.zeros((256, d), np.float32), None)
        for l, ids in enumerate(self.lists):
            if len(ids):
                assert self.o.add_keys(l, ids, np.zeros((len(ids), 1), np.uint8))
        self.o.set_raw(self.raw)


def shard_oracle(c, owner, w):
    """an oracle that holds the lists member w owns, and every row"""
    o = B.OracleIVFPQ(c.d, c.nlist, 1, 8, c.metric)
    o.set_trained(c.cc, np.zeros((256, c.d), np.float32), None)
    for l, ids in enumerate(c.lists):
        if owner[l] == w and len(ids):
            assert o.add_keys(l, ids, np.zeros((len(ids), 1), np.uint8))
    o.set_raw(c.raw)
    return o


def _pop_push(vals, ids, k, l2):
    vals = np.ascontiguousarray(vals, dtype=np.float32)
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    sv, si = np.empty(k, np.float32), np.empty(k, np.int64)
    B.lib().go_heap_pop_push_stream(1 if l2 else 0, k, vals.size, B._fp(vals), B._ip(ids), B._fp(sv), B._ip(si))
    return sv, si


def sharded_search(c, q, k, P, W, owner, rule="full", lists=None, **ctx_kw):
    """(D, I, info) of the sharded path.  lists: the lists as the shards hold them (default: the case's).  info: `flagged` [nq]
    bool, `cross` [nq] bool = equal distances from lists of two different owners at the k cut, `shard_cut` [W][nq] bool = the
    shard's own k cut went through a group of equal distances"""
    lists = c.lists if lists is None else lists
    l2 = c.metric == B.METRIC_L2
    nq = len(q)
    ctx = B.make_ctx(**ctx_kw)
    # every candidate of every query with its exact distance (the oracle's bits), and the coarse assignment
    kbig = max(k, P * max(len(l) for l in lists))
    Dall, Iall, st = B.ivfflat_search(c.o, q, kbig, P, c.metric, ctx, want_stages=True)
    ci = st["coarse_idx"]
    shards = [shard_oracle(c, owner, w) for w in range(W)]
    tabs = [B.ivfflat_search(o, q, k, P, c.metric, B.make_ctx(**ctx_kw)) for o in shards]
    D = np.empty((nq, k), np.float32)
    I = np.empty((nq, k), np.int64)
    flagged = np.zeros(nq, bool)
    cross = np.zeros(nq, bool)
    shard_cut = np.zeros((W, nq), bool)
    neutral = np.float32(3.402823466e+38 if l2 else -3.402823466e+38)
    for qi in range(nq):
        dist = {int(i): v for v, i in zip(Dall[qi], Iall[qi]) if i >= 0}
        # the stream the reference's scanner sees: probes in coarse order, entries in list order; who owns each entry
        sv, si, so = [], [], []
        for l in ci[qi]:
            if l < 0:
                continue
            for vid in lists[l]:
                if int(vid) in dist:
                    sv.append(dist[int(vid)])
                    si.append(int(vid))
                    so.append(int(owner[l]))
        sv, si, so = np.array(sv, np.float32), np.array(si, np.int64), np.array(so, np.int64)
        # the shards' tables (valid entries), their cut flags
        cd, cid = [], []
        ends = []
        for w in range(W):
            Dw, Iw = tabs[w][0][qi], tabs[w][1][qi]
            ok = Iw >= 0
            cd.append(Dw[ok])
            cid.append(Iw[ok])
            full = ok.all()
            ends.append(Dw[k - 1] if full else None)
            if full:
                mine = sv[so == w]
                shard_cut[w, qi] = (mine == Dw[k - 1]).sum() > (Dw == Dw[k - 1]).sum()
        alld, alli = np.concatenate(cd), np.concatenate(cid)
        order = np.argsort(alld if l2 else -alld, kind="stable")[:k]      # (distance, shard, rank)
        md, mi = alld[order], alli[order]
        D[qi], I[qi] = neutral, -1
        D[qi, :len(md)], I[qi, :len(mi)] = md, mi
        flag = bool((md[1:] == md[:-1]).any())                                           # (a)
        if len(md) == k:
            vk = md[k - 1]
            flag = flag or (alld == vk).sum() > (md == vk).sum()                          # (b)
            flag = flag or any(e is not None and e == vk and shard_cut[w, qi] for w, e in enumerate(ends))   # (c)
            grp = sv == vk
            cross[qi] = grp.sum() > (md == vk).sum() and len(set(so[grp].tolist())) > 1
        flagged[qi] = flag
        if flag and rule == "full":
            rv, ri = _pop_push(sv, si, k, l2)
            D[qi], I[qi] = rv, ri
            D[qi][ri < 0] = neutral
    return D, I, dict(flagged=flagged, cross=cross, shard_cut=shard_cut, coarse_idx=ci)
