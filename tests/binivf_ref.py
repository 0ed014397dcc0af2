"""The binary IVF model (index/impl/gamma_index_binary_ivf.{h,cc} over faiss 1.7.1's IndexBinaryIVF) restated from numpy
and the heap streams the oracle exports -- the yardstick of tests/test_binivf_cpu.py and tests/test_gpu_binivf*.py.

  * Hamming distances: popcount of XOR, numpy;
  * IsValid + IsSimilarScoreValid (common/gamma_common_data.h:95-108, as oracle.binding.make_ctx states them);
  * coarse step: IndexBinaryFlat::search = `dis < top -> heap_replace_top` over the centroids in index order, heap_reorder
    (go_heap_stream, keep-smallest);
  * scan: GammaIVFBinaryScannerL2::scan_codes = `dis < simi[0] -> heap_pop + heap_push` over the valid entries inside the
    score window, probes in coarse order, entries in list order, heap_reorder (go_heap_pop_push_stream);
  * training: binary_to_real, the k-means of the oracle (niter 10, seed 1234, 256 points per centroid), real_to_binary.
With use_ref=True the same functions run on the compiled faiss of oracle/_ref (ref_heap_stream, ref_heap_pop_push_stream,
ref_kmeans)."""
import numpy as np

from oracle import binding as B

EMPTY_D = np.float32(2147483648.0)   # (float)INT32_MAX: what an empty slot of the int32 heap reads as a float
INT32_MAX = 2147483647
FLT_TINY = float(np.finfo(np.float32).tiny)
FLT_MAX = float(np.finfo(np.float32).max)
POP8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.int32)


def hamming(q, codes):
    """q [cs] uint8, codes [n, cs] uint8 -> int32 [n]"""
    return POP8[np.bitwise_xor(codes, q[None, :])].sum(axis=1).astype(np.int32)


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _i(a):
    return np.ascontiguousarray(a, dtype=np.int64)


def heap_replace_top_stream(vals, ids, k, use_ref=False):
    """faiss heap of the k smallest, `top > v -> heap_replace_top`, heap_reorder: (values, ids) best first"""
    vals, ids = _f(vals), _i(ids)
    hv, sv = np.empty(k, np.float32), np.empty(k, np.float32)
    hi, si = np.empty(k, np.int64), np.empty(k, np.int64)
    fn = B.ref().ref_heap_stream if use_ref else B.lib().go_heap_stream
    fn(1, k, vals.size, B._fp(vals), B._ip(ids), B._fp(hv), B._ip(hi), B._fp(sv), B._ip(si))
    return sv, si


def heap_pop_push_stream(vals, ids, k, use_ref=False):
    """faiss heap of the k smallest, `top > v -> heap_pop + heap_push`, heap_reorder"""
    vals, ids = _f(vals), _i(ids)
    sv, si = np.empty(k, np.float32), np.empty(k, np.int64)
    fn = B.ref().ref_heap_pop_push_stream if use_ref else B.lib().go_heap_pop_push_stream
    fn(1, k, vals.size, B._fp(vals), B._ip(ids), B._fp(sv), B._ip(si))
    return sv, si


def coarse(x, cc, nprobe, use_ref=False):
    """IndexBinaryFlat::search: (distances int32 [nq, nprobe], INT32_MAX padded; labels int64 [nq, nprobe], -1 padded)"""
    nq = x.shape[0]
    D = np.empty((nq, nprobe), np.int32)
    I = np.empty((nq, nprobe), np.int64)
    ids = np.arange(cc.shape[0], dtype=np.int64)
    for i in range(nq):
        sv, si = heap_replace_top_stream(hamming(x[i], cc).astype(np.float32), ids, nprobe, use_ref)
        I[i] = si
        D[i] = np.where(si < 0, INT32_MAX, np.where(si < 0, 0, sv).astype(np.int64))
    return D, I


class Filter:
    """GammaSearchCondition::IsValid on vector ids: docid = vid2doc[vid]; the delete bitmap (a set of docids); range
    results as (docids, b_not_in) pairs, every one must hold (MultiRangeQueryResults::Has)"""

    def __init__(self, deleted=None, ranges=None, vid2doc=None):
        self.deleted = None if deleted is None else np.asarray(sorted(set(int(v) for v in deleted)), np.int64)
        self.ranges = None if ranges is None else [(np.asarray(sorted(set(int(v) for v in d)), np.int64), bool(n))
                                                    for d, n in ranges]
        self.vid2doc = None if vid2doc is None else np.asarray(vid2doc, np.int64)

    def valid(self, vids):
        vids = np.asarray(vids, np.int64)
        doc = vids if self.vid2doc is None else np.where(vids < self.vid2doc.size,
                                                         self.vid2doc[np.minimum(vids, self.vid2doc.size - 1)], vids)
        ok = np.ones(vids.size, bool)
        if self.ranges is not None:
            for docs, b_not_in in self.ranges:
                lo, hi = (int(docs[0]), int(docs[-1])) if docs.size else (0, 0)
                inset = np.isin(doc, docs)
                if b_not_in:   # outside [min, max]: has; inside: not in the set
                    has = (doc < lo) | (doc > hi) | ~inset
                else:
                    has = inset
                ok &= has
        if self.deleted is not None:
            ok &= ~np.isin(doc, self.deleted)
        return ok


def resolve_nprobe(nprobe, nlist):
    """GammaIndexBinaryIVF::Search: the request's nprobe if it lies in (0, nlist], else the model's 20"""
    return nprobe if 0 < nprobe <= nlist else 20


def search(lists, cc, x, k, nprobe, min_score=None, max_score=None, filt=None, use_ref=False, rows=None):
    """lists: [(vids int64 [n], codes uint8 [n, cs])] per list, in list order.  rows: the query rows to restate (all).
    Returns (D float32 [len(rows), k], I int64 [len(rows), k])."""
    nlist = cc.shape[0]
    P = resolve_nprobe(nprobe, nlist)
    lo = FLT_TINY if min_score is None else min_score
    hi = FLT_MAX if max_score is None else max_score
    rows = np.arange(x.shape[0]) if rows is None else np.asarray(rows)
    _, probes = coarse(x[rows], cc, P, use_ref)
    D = np.empty((rows.size, k), np.float32)
    I = np.empty((rows.size, k), np.int64)
    for r, q in enumerate(rows):
        vals, ids = [], []
        for l in probes[r]:
            if l < 0:
                continue
            lv, lc = lists[int(l)]
            if lv.size == 0:
                continue
            keep = lv >= 0
            if filt is not None:
                keep &= filt.valid(lv)
            dis = hamming(x[q], lc).astype(np.float32)
            keep &= (dis <= np.float32(hi)) & (dis >= np.float32(lo))
            vals.append(dis[keep])
            ids.append(lv[keep])
        vals = np.concatenate(vals) if vals else np.empty(0, np.float32)
        ids = np.concatenate(ids) if ids else np.empty(0, np.int64)
        sv, si = heap_pop_push_stream(vals, ids, k, use_ref)
        D[r] = np.where(si < 0, EMPTY_D, sv)
        I[r] = si
    return D, I


def binary_to_real(codes):
    """faiss:utils/utils.cpp:634-638: bit i of byte i >> 3 -> 2 * bit - 1"""
    bits = np.unpackbits(np.ascontiguousarray(codes, np.uint8), axis=1, bitorder="little")
    return (2.0 * bits.astype(np.float32) - 1.0).astype(np.float32)


def real_to_binary(x):
    """faiss:utils/utils.cpp:640-650: bit set only for a component > 0 (0.0 gives 0)"""
    return np.packbits((np.asarray(x) > 0).astype(np.uint8), axis=1, bitorder="little")


def train(codes, nlist, use_ref=False):
    """IndexBinaryIVF::train as GammaIndexBinaryIVF::Indexing runs it: centroid codes [nlist, cs]"""
    x = binary_to_real(codes)
    if use_ref:
        cen = np.empty((nlist, x.shape[1]), np.float32)
        B.ref().ref_kmeans(x.shape[1], x.shape[0], B._fp(x), nlist, 10, 1234, B._fp(cen))
    else:
        cen, _ = B.kmeans(x, nlist, 10, seed=1234, max_points_per_centroid=256)
    return real_to_binary(cen)


def assign_lists(codes, cc, first_vid=0, lists=None):
    """Add: quantizer->assign (k = 1: the lowest centroid index among equal distances), AddKeys in vid order"""
    nlist, cs = cc.shape
    if lists is None:
        lists = [(np.empty(0, np.int64), np.empty((0, cs), np.uint8)) for _ in range(nlist)]
    _, a = coarse(codes, cc, 1)
    a = a[:, 0]
    out = []
    for l in range(nlist):
        sel = np.nonzero(a == l)[0]
        v, c = lists[l]
        out.append((np.concatenate([v, first_vid + sel.astype(np.int64)]), np.concatenate([c, codes[sel]])))
    return out


def clustered_codes(n, nbits, ncenters, flip=0.05, seed=0, dup_frac=0.05):
    """Clustered codes with few flipped bits, plus exact duplicates of earlier rows"""
    rng = np.random.default_rng(seed)
    cs = nbits // 8
    centers = rng.integers(0, 256, size=(ncenters, cs), dtype=np.uint8)
    bits = np.unpackbits(centers[rng.integers(0, ncenters, n)], axis=1, bitorder="little")
    bits ^= (rng.random(bits.shape) < flip).astype(np.uint8)
    codes = np.packbits(bits, axis=1, bitorder="little")
    ndup = int(n * dup_frac)
    if ndup and n > 1:
        dst = rng.integers(1, n, ndup)
        codes[dst] = codes[(rng.random(ndup) * dst).astype(np.int64)]
    return np.ascontiguousarray(codes)
