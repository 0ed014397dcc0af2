"""Data of the tests of the row-sliced list-major IVFFLAT scan (tests/test_gpu_ivfflat_lm_anyd.py, tests/test_ivfflat_lm_cpu.py,
DESIGN section 22): the cases of tests/ivfflat_rows_data.py with fp32 rows beside the narrow ones and with lists of chosen
lengths, and what the CPU can say about a case before the GPU sees it (probing queries per list, work units)."""
import numpy as np

from oracle import binding as B
from tests import ivfflat_rows_data as R

MANY_P = 4
EDGE_128, EDGE_129, EDGE_EMPTY = 2, 9, 5
TIE_K = 20
GRID_P = 16


class Case(R.Case):
    """R.Case with dtype "float32" as well (rows of full fp32 precision: W is base) and, with `sizes` = {list: length}, lists
    of exactly those lengths: rows move between the named lists and the longest others (any assignment serves, the oracle and
    the handles hold the SAME lists)"""

    def __init__(self, d, dtype, metric, N=3001, nlist=16, nq=33, seed=0, empty=None, ties=False, sizes=None):
        self.d, self.dtype, self.metric, self.nlist, self.N = d, dtype, metric, nlist, N
        if dtype == "float32":
            rng = np.random.default_rng(100 + seed)      # 40 prototypes plus noise, as the byte rows: lists of similar lengths
            proto = 3 * rng.standard_normal((40, d))
            self.base = (proto[rng.integers(0, 40, N)] + 0.75 * rng.standard_normal((N, d))).astype(np.float32)
            self.W = self.base
            qkind = "float16"      # (R.queries: the noise scale of normal rows)
        else:
            self.base = R.tie_rows(N, d, dtype, 100 + seed) if ties else R.base_rows(N, d, dtype, 100 + seed)
            self.W = R.widened(self.base, dtype)
            qkind = dtype
        self.cc = R.centroids(self.W, nlist, 200 + seed)
        self.q = R.queries(nq, d, qkind, 300 + seed, self.W)
        lno = R.assign(self.W, self.cc, empty)
        for l, want in (sizes or {}).items():
            fixed = set(sizes) | ({empty} if empty is not None else set())
            while (lno == l).sum() != want:
                others = [m for m in range(nlist) if m not in fixed]
                big = max(others, key=lambda m: (lno == m).sum())
                if (lno == l).sum() > want:
                    lno[np.flatnonzero(lno == l)[-1]] = big
                else:
                    lno[np.flatnonzero(lno == big)[-1]] = l
        order = np.argsort(lno, kind="stable")
        self.lists = [order[lno[order] == l].astype(np.int64) for l in range(nlist)]
        self.raw = self.W.copy()
        self.o = B.OracleIVFPQ(d, nlist, 1, 8, metric)
        self.o.set_trained(self.cc, np.zeros((256, d), np.float32), None)
        for l, ids in enumerate(self.lists):
            if len(ids):
                assert self.o.add_keys(l, ids, np.zeros((len(ids), 1), np.uint8))
        self.o.set_raw(self.raw)


def probes_per_list(c, q, P):
    """how many of the queries probe each list, from the oracle's coarse assignment"""
    _, _, st = B.ivfflat_search(c.o, q, 1, P, c.metric, B.make_ctx(), want_stages=True)
    ci = st["coarse_idx"]
    return np.bincount(ci[ci >= 0].astype(np.int64), minlength=c.nlist)


def work_units(c, q, P, qtile):
    """the work units of the list-major scan: per non-empty probed list, query tiles x 128-row chunks"""
    cnt = probes_per_list(c, q, P)
    return int(sum(-(-int(n) // qtile) * -(-len(c.lists[l]) // 128) for l, n in enumerate(cnt) if len(c.lists[l])))


def many_queries_case(qtile):
    """40 queries drawn around three centroids, qtile + 1 | qtile | the rest: the first centroid's list is probed by more than
    one tile of queries and a list only the second group probes by exactly one full tile.  The centroids are the first triple
    (in a fixed order) for which the oracle's assignment says so; returns (case, queries)."""
    c = Case(144, "float32", B.METRIC_L2, seed=11)
    rng = np.random.default_rng(411)
    noise = 0.01 * rng.standard_normal((40, c.d)).astype(np.float32)
    groups = np.repeat([0, 1, 2], [qtile + 1, qtile, 40 - 2 * qtile - 1])
    for a in range(c.nlist):
        for b in range(c.nlist):
            for e in range(c.nlist):
                if len({a, b, e}) < 3:
                    continue
                q = np.ascontiguousarray(c.cc[np.array([a, b, e])[groups]] + noise)
                cnt = probes_per_list(c, q, MANY_P)
                if (cnt > qtile).any() and (cnt == qtile).any():
                    return c, q
    raise AssertionError("no triple of centroids gives the per-list counts the case needs")


def edge_case(dtype="float32", seed=19):
    """a list of exactly 128 rows (one full chunk), one of 129 (a chunk of one row), an empty one that queries probe"""
    return Case(144, dtype, B.METRIC_L2, empty=EDGE_EMPTY, seed=seed, sizes={EDGE_128: 128, EDGE_129: 129})


def tie_case():
    """integer-valued rows, every distinct row four times: equal distances among a query's results"""
    return Case(144, "uint8", B.METRIC_L2, ties=True, seed=13)


def grid_case():
    """nlist 64, lists of about 400 rows, 600 queries x 16 probes: more work units than the 2048 persistent workgroups"""
    return Case(144, "float32", B.METRIC_L2, N=25600, nlist=64, nq=600, seed=14)
