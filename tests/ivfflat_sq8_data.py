"""Data of the IVFFLAT-over-sq8-rows tests (tests/test_gpu_ivfflat_sq8*.py, tests/test_ivfflat_sq8_cpu.py):
rows, ranges, queries, centroids and lists that the CPU test can examine and the GPU tests then use unchanged.

base is what a caller hands to the store: float rows, 40 prototypes plus noise (lists of similar lengths) under a scale and an
offset of their own per dimension (tests/sq8_ref.py's: magnitudes over three decades, every third dimension negative throughout).
The ranges are the minimum / maximum of the FIRST HALF of the rows; the second half is drawn 1.6 times as wide and clips at both
ends, and one dimension is constant over the first half (vmin == vmax, step 0: every row decodes to the constant there).
W = sq8_ref.stored(base, vmin, vmax) is what the store holds; lists are by W's nearest centroid (any assignment serves: the oracle
and the handles hold the SAME lists)."""
import numpy as np

from oracle import binding as B
from tests import ivfflat_rows_data as R
from tests import sq8_ref as S

TIE_K = R.TIE_K            # 10: TIE_COPIES does not divide it, so a group of equal rows straddles the cut
TIE_COPIES = R.TIE_COPIES  # 4


def dim_params(d):
    """(scale, offset, constant dimension) of a row length: sq8_ref.rows's"""
    p = np.random.default_rng(1000 + d)
    scale = 10.0 ** p.uniform(-2.0, 1.0, d)
    offset = p.uniform(-3.0, 3.0, d) * scale
    offset[::3] = -8.0 * scale[::3]
    return scale, offset, min(5, d - 1)


def base_rows(n, d, seed):
    """(rows, vmin, vmax): the caller's fp32 rows and the ranges of their first half"""
    scale, offset, cd = dim_params(d)
    rng = np.random.default_rng(seed)
    proto = 3.0 * rng.standard_normal((40, d))
    wide = np.where(np.arange(n) < n // 2, 1.0, 1.6)[:, None]
    x = offset + scale * wide * (proto[rng.integers(0, 40, n)] + 0.75 * rng.standard_normal((n, d)))
    x[:, cd] = 0.75
    x[n // 2:, cd] += 0.1 * rng.standard_normal(n - n // 2)      # varies where the ranges do not look
    x = np.ascontiguousarray(x, dtype=np.float32)
    return x, x[:n // 2].min(axis=0), x[:n // 2].max(axis=0)


def tie_rows(n, d, seed):
    """every distinct row TIE_COPIES times (one of them once more), shuffled; the ranges are those of the distinct rows' first
    half.  Copies of a row encode to the same codes, share a list and a distance to any query."""
    distinct, vmin, vmax = base_rows(n // TIE_COPIES, d, seed)
    pick = np.arange(n) % len(distinct)
    np.random.default_rng(seed + 1).shuffle(pick)
    return np.ascontiguousarray(distinct[pick]), vmin, vmax


def queries(nq, d, seed, W):
    """queries near rows of W, not on them"""
    scale, _, _ = dim_params(d)
    rng = np.random.default_rng(seed)
    return (W[rng.integers(0, len(W), nq)] + 0.5 * scale * rng.standard_normal((nq, d))).astype(np.float32)


def centroids(W, nlist, seed):
    scale, _, _ = dim_params(W.shape[1])
    rng = np.random.default_rng(seed)
    pick = rng.choice(len(W), nlist, replace=False)
    return np.ascontiguousarray(W[pick] + 0.25 * scale * rng.standard_normal((nlist, W.shape[1])), dtype=np.float32)


class Case:
    """rows, ranges, lists and an oracle that holds the lists with set_raw(W).  sizes = {list: length}: lists of exactly those
    lengths (rows move between the named lists and the longest others); empty: a list that gets nothing yet stays probed."""

    def __init__(self, d, metric, N=3001, nlist=16, nq=33, seed=0, empty=None, ties=False, sizes=None):
        self.d, self.metric, self.nlist, self.N = d, metric, nlist, N
        self.base, self.vmin, self.vmax = (tie_rows if ties else base_rows)(N, d, 100 + seed)
        self.W = np.ascontiguousarray(S.stored(self.base, self.vmin, self.vmax))
        self.cc = centroids(self.W, nlist, 200 + seed)
        self.q = queries(nq, d, 300 + seed, self.W)
        lno = R.assign(self.W, self.cc, empty)
        fixed = set(sizes or {}) | ({empty} if empty is not None else set())
        for l, want in (sizes or {}).items():
            while (lno == l).sum() != want:
                big = max((m for m in range(nlist) if m not in fixed), key=lambda m: (lno == m).sum())
                if (lno == l).sum() > want:
                    lno[np.flatnonzero(lno == l)[-1]] = big
                else:
                    lno[np.flatnonzero(lno == big)[-1]] = l
        order = np.argsort(lno, kind="stable")
        self.lists = [order[lno[order] == l].astype(np.int64) for l in range(nlist)]
        self.raw = self.W.copy()      # what the oracle reads; follows the writers
        self.o = B.OracleIVFPQ(d, nlist, 1, 8, metric)
        self.o.set_trained(self.cc, np.zeros((256, d), np.float32), None)
        for l, ids in enumerate(self.lists):
            if len(ids):
                assert self.o.add_keys(l, ids, np.zeros((len(ids), 1), np.uint8))
        self.o.set_raw(self.raw)

    def stored(self, x):
        """what the store holds for rows x"""
        return np.ascontiguousarray(S.stored(x, self.vmin, self.vmax))

    def load(self, g):
        """the lists into a handle (initialised for IVFFLAT, any store)"""
        used = [l for l in range(self.nlist) if len(self.lists[l])]
        vids = np.concatenate([self.lists[l] for l in used])
        g.add_keys_batch(used, [len(self.lists[l]) for l in used], vids, np.zeros((len(vids), 1), np.uint8))

    def oracle(self, q, k, P, **ctx_kw):
        return B.ivfflat_search(self.o, q, k, P, self.metric, B.make_ctx(**ctx_kw))


def probes_per_list(c, q, P):
    """how many of the queries probe each list, from the oracle's coarse assignment"""
    _, _, st = B.ivfflat_search(c.o, q, 1, P, c.metric, B.make_ctx(), want_stages=True)
    ci = st["coarse_idx"]
    return np.bincount(ci[ci >= 0].astype(np.int64), minlength=c.nlist)


EDGE_128, EDGE_129, EDGE_EMPTY = 2, 9, 5


def edge_case(d=144, seed=19):
    """a list of exactly 128 rows (one full chunk), one of 129 (a chunk of one row), an empty one that queries probe"""
    return Case(d, B.METRIC_L2, empty=EDGE_EMPTY, seed=seed, sizes={EDGE_128: 128, EDGE_129: 129})
