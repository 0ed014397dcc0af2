"""The IVFPQ model with 4-bit codes (nbits_per_idx = 4: faiss::ProductQuantizer with ksub = 16, PQEncoderGeneric /
PQDecoderGeneric, under GammaIVFPQIndex's search, index/impl/gamma_index_ivfpq.{h,cc}) restated from numpy and the
primitives the oracle exports with `ksub` -- the yardstick of tests/test_pq4_cpu.py and tests/test_gpu_pq4*.py.  The oracle's
own index (go_ivfpq_new) is 8-bit only; its primitives are not:

  * tables: go_ivfpq_precompute_table, go_pq_inner_prod_table, go_fvec_madd (ksub = 16);
  * codes: go_pq_compute_codes gives one index per byte, packed here as PQEncoderGeneric packs them
    (faiss:impl/ProductQuantizer-inl.h:10-44): sub-quantizer m in bits [4m, 4m + 4), an odd M leaves the last high nibble 0;
  * coarse step: go_knn_L2sqr (mode 0 below 20 queries, the BLAS form from 20 on, as faiss decides);
  * scan: dis = dis0, then `dis += table[m][nibble_m]` for m ascending (sequential fp32 adds), fed in probe and list order
    into the recall heap: `top > dis -> heap_replace_top` (go_heap_stream: the heap ARRAY and its sorted form);
  * compute_dis in the order oracle/gamma_oracle.c:1120-1147 uses: with rank, the exact distances of the heap array's
    entries inside the score window through `top > dis -> heap_pop + heap_push` (go_heap_pop_push_stream); without, the
    first k entries of the sorted recall heap inside the score window;
  * training: go_kmeans for the coarse centroids, residuals of at most 256 * 16 points (go_rand_perm, seed 1234),
    go_kmeans(dsub, 16, niter 25) per sub-quantizer (faiss:IndexIVFPQ.cpp:67-131);
  * filters as tests/binivf_ref.Filter states them; bit 63 of a list id = superseded by an Update.
With use_ref=True the heap streams and k-means run on the compiled faiss of oracle/_ref."""
import ctypes as C

import numpy as np

from oracle import binding as B
from tests.binivf_ref import Filter  # noqa: F401  (re-exported: the tests build their filters from it)

KSUB = 16
FLT_TINY = float(np.finfo(np.float32).tiny)
FLT_MAX = float(np.finfo(np.float32).max)
DEL_MASK = np.int64(-2 ** 63)


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _i(a):
    return np.ascontiguousarray(a, dtype=np.int64)


def code_size(M):
    return (4 * M + 7) // 8


def pack(idx):
    """[n, M] indices < 16 -> [n, code_size] bytes"""
    idx = np.ascontiguousarray(idx, dtype=np.uint8)
    n, M = idx.shape
    assert (idx < KSUB).all()
    pad = np.zeros((n, 2 * code_size(M)), np.uint8)
    pad[:, :M] = idx
    return np.ascontiguousarray(pad[:, 0::2] | (pad[:, 1::2] << 4))


def unpack(codes, M):
    """[n, code_size] bytes -> [n, M] indices"""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    out = np.empty((codes.shape[0], 2 * codes.shape[1]), np.uint8)
    out[:, 0::2] = codes & 15
    out[:, 1::2] = codes >> 4
    return np.ascontiguousarray(out[:, :M])


def precompute_table(cc, pq):
    """T2 [nlist, M, 16] (faiss:IndexIVFPQ.cpp:453-479)"""
    cc, pq = _f(cc), _f(pq)
    nlist, d = cc.shape
    M = pq.shape[0]
    assert pq.shape == (M, KSUB, d // M)
    out = np.empty((nlist, M, KSUB), np.float32)
    B.lib().go_ivfpq_precompute_table(B._fp(cc), nlist, d, B._fp(pq), M, KSUB, B._fp(out))
    return out


def ip_table(pq, x):
    """[M, 16] inner products of one query's sub-vectors with the codebooks"""
    pq, x = _f(pq), _f(x)
    M, _, dsub = pq.shape
    out = np.empty((M, KSUB), np.float32)
    B.lib().go_pq_inner_prod_table(B._fp(pq), M, KSUB, dsub, B._fp(x), B._fp(out))
    return out


def assign(x, cc, mode=None):
    """quantizer->assign: the exact form below 20 vectors, the BLAS form from 20 on (mode 0 / 1 forces one)"""
    x = _f(x)
    if mode is None:
        mode = 0 if x.shape[0] < 20 else 1
    _, a = B.knn_L2sqr(x, cc, 1, mode)
    return a[:, 0]


def encode(x, cc, pq, mode=None):
    """(list_nos int64 [n], packed codes uint8 [n, code_size]): residual to the assigned centroid, compute_codes"""
    x, cc, pq = _f(x), _f(cc), _f(pq)
    M, _, dsub = pq.shape
    lno = assign(x, cc, mode)
    res = _f(x - cc[lno])
    idx = np.empty((x.shape[0], M), np.uint8)
    B.lib().go_pq_compute_codes(B._fp(pq), M, KSUB, dsub, B._fp(res), B._up(idx), x.shape[0])
    return lno.astype(np.int64), pack(idx)


def encode_each(x, cc, pq):
    """every vector assigned as a call of its own (GammaIVFPQIndex::Update)"""
    return encode(x, cc, pq, mode=0)


def build_lists(lno, codes, nlist, first_vid=0, lists=None):
    """Add: AddKeys per list in ascending list order, vids in arrival order"""
    cs = codes.shape[1]
    if lists is None:
        lists = [(np.empty(0, np.int64), np.empty((0, cs), np.uint8)) for _ in range(nlist)]
    out = []
    for l in range(nlist):
        sel = np.nonzero(lno == l)[0]
        v, c = lists[l]
        out.append((np.concatenate([v, first_vid + sel.astype(np.int64)]), np.concatenate([c, codes[sel]])))
    return out


def train(x, nlist, M, use_ref=False):
    """IndexIVFPQ::train as GammaIVFPQIndex::Indexing configures it, with pq.ksub = 16: (coarse [nlist, d], pq [M, 16, dsub])"""
    x = _f(x)
    n, d = x.shape
    dsub = d // M

    def km(v, k, niter):
        if use_ref:
            cen = np.empty((k, v.shape[1]), np.float32)
            B.ref().ref_kmeans(v.shape[1], v.shape[0], B._fp(v), k, niter, 1234, B._fp(cen))
            return cen
        return B.kmeans(v, k, niter, seed=1234, max_points_per_centroid=256)[0]

    cc = km(x, nlist, 10)
    nmax = 256 * KSUB
    xs = x
    if n > nmax:
        perm = np.empty(n, np.int32)
        B.lib().go_rand_perm(perm.ctypes.data_as(C.POINTER(C.c_int)), n, 1234)
        xs = _f(x[perm[:nmax]])
    a = assign(xs, cc)
    res = _f(xs - cc[a])
    pq = np.empty((M, KSUB, dsub), np.float32)
    for m in range(M):
        pq[m] = km(_f(res[:, m * dsub:(m + 1) * dsub]), KSUB, 25)
    return cc, pq


def coarse(x, cc, nprobe, mode=None):
    x = _f(x)
    if mode is None:
        mode = 0 if x.shape[0] < 20 else 1
    return B.knn_L2sqr(x, cc, nprobe, mode)


def heap_stream(vals, ids, k, l2, use_ref=False):
    """`top > v -> heap_replace_top` over the stream: (heap array values, ids, sorted values, ids); empty slots id -1"""
    vals, ids = _f(vals), _i(ids)
    hv, sv = np.empty(k, np.float32), np.empty(k, np.float32)
    hi, si = np.empty(k, np.int64), np.empty(k, np.int64)
    fn = B.ref().ref_heap_stream if use_ref else B.lib().go_heap_stream
    fn(1 if l2 else 0, k, vals.size, B._fp(vals), B._ip(ids), B._fp(hv), B._ip(hi), B._fp(sv), B._ip(si))
    return hv, hi, sv, si


def heap_pop_push_stream(vals, ids, k, l2, use_ref=False):
    vals, ids = _f(vals), _i(ids)
    sv, si = np.empty(k, np.float32), np.empty(k, np.int64)
    fn = B.ref().ref_heap_pop_push_stream if use_ref else B.lib().go_heap_pop_push_stream
    fn(1 if l2 else 0, k, vals.size, B._fp(vals), B._ip(ids), B._fp(sv), B._ip(si))
    return sv, si


def _exact(l2, xq, rows):
    out = np.empty(rows.shape[0], np.float32)
    fn = B.lib().go_fvec_L2sqr if l2 else B.lib().go_fvec_inner_product
    d = xq.size
    for i in range(rows.shape[0]):
        out[i] = fn(B._fp(xq), B._fp(rows[i]), d)
    return out


class Index:
    """Trained state + lists [(ids int64 [n] with bit 63 = superseded, packed codes [n, code_size])] + raw vectors"""

    def __init__(self, cc, pq, lists, raw=None, table=None):
        self.cc, self.pq = _f(cc), _f(pq)
        self.nlist, self.d = self.cc.shape
        self.M = self.pq.shape[0]
        self.T2 = precompute_table(cc, pq) if table is None else _f(table)
        self.lists = lists
        self.raw = None if raw is None else _f(raw)

    def adc(self, l2, xq, probes, cdis, filt=None):
        """the scan's stream of one query: (distances, vids) of the valid entries in probe and list order"""
        M, tsz = self.M, self.M * KSUB
        ipt = ip_table(self.pq, xq).reshape(-1)
        tab = np.empty(tsz, np.float32)
        mi = np.arange(M)
        vals, ids = [], []
        for ik, key in enumerate(probes):
            key = int(key)
            if key < 0 or key >= self.nlist:
                continue
            lv, lc = self.lists[key]
            if lv.size == 0:
                continue
            if l2:
                dis0 = np.float32(cdis[ik])
                B.lib().go_fvec_madd(tsz, B._fp(_f(self.T2[key].reshape(-1))), -2.0, B._fp(ipt), B._fp(tab))
                t = tab.reshape(M, KSUB)
            else:
                dis0 = np.float32(B.lib().go_fvec_inner_product(B._fp(xq), B._fp(_f(self.cc[key])), self.d))
                t = ipt.reshape(M, KSUB)
            keep = lv >= 0
            if filt is not None:
                keep &= filt.valid(lv & ~DEL_MASK)
            idx = unpack(lc[keep], M)
            dis = np.full(idx.shape[0], dis0, np.float32)
            for m in mi:   # sequential fp32 adds, m ascending
                dis = (dis + t[m][idx[:, m]]).astype(np.float32)
            vals.append(dis)
            ids.append(lv[keep])
        if not vals:
            return np.empty(0, np.float32), np.empty(0, np.int64)
        return np.concatenate(vals), np.concatenate(ids)

    def search(self, x, k, nprobe, recall_num=100, has_rank=True, l2=True, min_score=None, max_score=None, filt=None,
               coarse_mode=None, preassigned=None, use_ref=False, rows=None):
        """GammaIVFPQIndex::Search.  Returns (D [n, k], I [n, k], stages) for the query rows `rows` (all); the coarse
        step always runs over the whole batch (its arithmetic form depends on the batch size).  Empty slots: id -1."""
        x = _f(x)
        R = max(recall_num, k)
        lo = FLT_TINY if min_score is None else min_score
        hi = FLT_MAX if max_score is None else max_score
        if preassigned is not None:
            cd, ci = _f(preassigned[0]), _i(preassigned[1])
        else:
            cd, ci = coarse(x, self.cc, nprobe, coarse_mode)
        rows = np.arange(x.shape[0]) if rows is None else np.asarray(rows)
        neutral = np.float32(FLT_MAX if l2 else -FLT_MAX)
        D = np.full((rows.size, k), neutral, np.float32)
        I = np.full((rows.size, k), -1, np.int64)
        rd = np.empty((rows.size, R), np.float32)
        ri = np.empty((rows.size, R), np.int64)
        for r, q in enumerate(rows):
            vals, ids = self.adc(l2, x[q], ci[q], cd[q], filt)
            hv, hid, sv, sid = heap_stream(vals, ids, R, l2, use_ref)
            rd[r], ri[r] = sv, sid
            if has_rank:
                live = hid != -1
                ex = _exact(l2, x[q], self.raw[hid[live]])
                ok = (ex <= np.float32(hi)) & (ex >= np.float32(lo))
                fv, fi = heap_pop_push_stream(ex[ok], hid[live][ok], k, l2, use_ref)
                D[r], I[r] = fv, fi
            else:
                live = sid != -1
                ok = (sv[live] <= np.float32(hi)) & (sv[live] >= np.float32(lo))
                tv, ti = sv[live][ok][:k], sid[live][ok][:k]
                D[r, :tv.size], I[r, :ti.size] = tv, ti
        return D, I, dict(coarse_dis=cd[rows], coarse_idx=ci[rows], recall_dis=rd, recall_ids=ri)

    # ---- realtime lists (realtime/realtime_mem_data.cc) on the yardstick's own arrays -------------------------
    def find(self, vid):
        for l, (lv, _) in enumerate(self.lists):
            pos = np.nonzero(lv == vid)[0]
            if pos.size:
                return l, int(pos[0])
        return None

    def update(self, vid, vec):
        """GammaIVFPQIndex::Update of one vector: same list -> the code is rewritten; else the old slot gets bit 63 and
        the entry is appended to the new list"""
        lno, code = encode_each(_f(vec)[None, :], self.cc, self.pq)
        at = self.find(vid)
        if at is None:
            return
        l, pos = at
        nl = int(lno[0])
        if nl == l:
            self.lists[l][1][pos] = code[0]
            return
        self.lists[l][0][pos] |= DEL_MASK
        v, c = self.lists[nl]
        self.lists[nl] = (np.concatenate([v, np.asarray([vid], np.int64)]), np.concatenate([c, code]))

    def compact(self, l, deleted_docs=()):
        """CompactBucket: entries without bit 63 whose doc is not deleted, in order"""
        lv, lc = self.lists[l]
        keep = (lv >= 0) & ~np.isin(lv, np.asarray(list(deleted_docs), np.int64))
        self.lists[l] = (lv[keep].copy(), lc[keep].copy())


def clustered(n, d, seed, ncenters=40, integer=False):
    """clustered float data; integer=True: small integer coordinates (exact ADC / exact-distance ties)"""
    rng = np.random.default_rng(seed)
    if integer:
        cen = rng.integers(-4, 5, size=(ncenters, d))
        x = cen[rng.integers(0, ncenters, n)] + rng.integers(-1, 2, size=(n, d))
        return x.astype(np.float32)
    cen = rng.normal(size=(ncenters, d)).astype(np.float32) * 4
    return (cen[rng.integers(0, ncenters, n)] + rng.normal(size=(n, d)).astype(np.float32)).astype(np.float32)
