"""Data of the IVFFLAT-over-narrow-rows tests (tests/test_gpu_ivfflat_rows*.py, tests/test_ivfflat_rows_cpu.py): rows, queries,
centroids and lists that the CPU test can examine and the GPU tests then use unchanged.

base is what a caller hands to the store, W = base.astype(T).astype(float32) what the store of type T holds.  Byte rows are
prototypes plus small integer noise (W == base: integers convert exactly); float16 rows are scaled normals, whose rounding to
half is NOT the identity (W != base)."""
import numpy as np

from oracle import binding as B

DTYPES = ["float16", "uint8", "int8"]
NP = {"float16": np.float16, "uint8": np.uint8, "int8": np.int8}
RANGE = {"uint8": (0, 255), "int8": (-128, 127)}
ESZ = {"float16": 2, "uint8": 1, "int8": 1}
TIE_K = 10      # the k of the tie cases: TIE_COPIES does not divide it, so a group of equal rows straddles the cut
TIE_COPIES = 4


def widened(x, dtype):
    """W: what the store of this type holds for x, as fp32 (x must be inside the type's range)"""
    return np.ascontiguousarray(x.astype(NP[dtype]).astype(np.float32))


def base_rows(n, d, dtype, seed):
    """the rows as the caller has them, fp32"""
    rng = np.random.default_rng(seed)
    if dtype == "float16":
        return (rng.standard_normal((n, d)) * 3).astype(np.float32)
    lo, hi = RANGE[dtype]
    proto = rng.integers(lo + 8, hi - 8, size=(40, d))
    x = proto[rng.integers(0, 40, n)] + rng.integers(-8, 9, size=(n, d))
    x[0, 0], x[0, -1] = lo, hi
    return x.astype(np.float32)


def queries(nq, d, dtype, seed, W):
    """queries near rows of W, not on them"""
    rng = np.random.default_rng(seed)
    scale = 0.5 if dtype == "float16" else 6.0
    return (W[rng.integers(0, len(W), nq)] + scale * rng.standard_normal((nq, d))).astype(np.float32)


def tie_rows(n, d, dtype, seed):
    """every distinct row TIE_COPIES times (one of them once more), shuffled: the copies of a row share its list and its
    distance to any query, so ranks 8 .. 11 of a query are one group and k = TIE_K cuts it"""
    distinct = base_rows(n // TIE_COPIES, d, dtype, seed)
    pick = np.arange(n) % len(distinct)
    np.random.default_rng(seed + 1).shuffle(pick)
    return np.ascontiguousarray(distinct[pick])


def centroids(W, nlist, seed):
    rng = np.random.default_rng(seed)
    pick = rng.choice(len(W), nlist, replace=False)
    return np.ascontiguousarray(W[pick] + 0.25 * rng.standard_normal((nlist, W.shape[1])).astype(np.float32), dtype=np.float32)


def assign(W, cc, empty=None):
    """nearest centroid (any assignment serves: the oracle and the handles hold the SAME lists); `empty`: a list that gets
    nothing -- its members go to their next centroid -- yet stays among the probed ones"""
    W64, c64 = W.astype(np.float64), cc.astype(np.float64)
    dis = (W64 ** 2).sum(1)[:, None] - 2.0 * W64 @ c64.T + (c64 ** 2).sum(1)[None, :]
    if empty is not None:
        dis[:, empty] = np.inf
    return np.argmin(dis, axis=1)


class Case:
    """rows, lists and an oracle that holds them with set_raw(W)"""

    def __init__(self, d, dtype, metric, N=3001, nlist=16, nq=33, seed=0, empty=None, ties=False):
        self.d, self.dtype, self.metric, self.nlist, self.N = d, dtype, metric, nlist, N
        self.base = tie_rows(N, d, dtype, 100 + seed) if ties else base_rows(N, d, dtype, 100 + seed)
        self.W = widened(self.base, dtype)
        self.cc = centroids(self.W, nlist, 200 + seed)
        self.q = queries(nq, d, dtype, 300 + seed, self.W)
        lno = assign(self.W, self.cc, empty)
        order = np.argsort(lno, kind="stable")
        self.lists = [order[lno[order] == l].astype(np.int64) for l in range(nlist)]
        self.raw = self.W.copy()      # what the oracle reads; follows the writers
        self.o = B.OracleIVFPQ(d, nlist, 1, 8, metric)
        self.o.set_trained(self.cc, np.zeros((256, d), np.float32), None)
        for l, ids in enumerate(self.lists):
            if len(ids):
                assert self.o.add_keys(l, ids, np.zeros((len(ids), 1), np.uint8))
        self.o.set_raw(self.raw)

    def load(self, g):
        """the lists into a handle (initialised for IVFFLAT, any store)"""
        used = [l for l in range(self.nlist) if len(self.lists[l])]
        vids = np.concatenate([self.lists[l] for l in used])
        g.add_keys_batch(used, [len(self.lists[l]) for l in used], vids, np.zeros((len(vids), 1), np.uint8))

    def oracle(self, q, k, P, **ctx_kw):
        return B.ivfflat_search(self.o, q, k, P, self.metric, B.make_ctx(**ctx_kw))
