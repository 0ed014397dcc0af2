"""GPU: seeded random 4-bit IVFPQ configurations -- shapes, metrics, deletes, range filters, score windows, recall_num on
both sides of k -- strictly against the yardstick (tests/pq4_ref.py).
Seeds: GAMMA_PQ4_FUZZ_SEEDS (comma-separated; default a small fixed set)."""
import os

import numpy as np
import pytest

from gamma_amd import api
from tests import pq4_ref as PR
from tests.parity import compare_search_exact

pytestmark = pytest.mark.gpu

SEEDS = [int(s) for s in os.environ.get("GAMMA_PQ4_FUZZ_SEEDS", "1,2,3,4,5,6").split(",") if s.strip()]


@pytest.mark.parametrize("seed", SEEDS)
def test_pq4_fuzz(seed):
    rng = np.random.default_rng(seed)
    M = int(rng.choice([1, 2, 3, 5, 8, 12, 16, 24, 32, 64]))
    dsub = int(rng.choice([1, 2, 3, 4, 8, 12, 16]))
    dsub = max(1, min(dsub, 384 // M))   # d <= 384: the GEMM-form coarse distances beyond are not restated bit for bit
    d = M * dsub
    nlist = int(rng.choice([9, 16, 32]))
    N = int(rng.integers(600, 3000))
    integer = bool(rng.integers(0, 2))
    base = PR.clustered(N, d, seed, integer=integer)
    cc, pq = PR.train(base, nlist, M)
    l2_index = bool(rng.integers(0, 2))
    g = api.GammaHip(0)
    try:
        g.ivfpq4_init(d, nlist, M, api.METRIC_L2 if l2_index else api.METRIC_IP, int(rng.integers(1, 1500)))
        g.ivfpq_set_trained(cc, pq, None)
        g.raw_init(d)
        g.raw_append(base)
        lists = None
        i0 = 0
        while i0 < N:   # Add in batches of random size (fewer than 20 vectors take the exact assignment)
            n = int(min(N - i0, rng.choice([5, 19, 20, 333, 1000])))
            g.add(base[i0:i0 + n], i0)
            lno, codes = PR.encode(base[i0:i0 + n], cc, pq)
            lists = PR.build_lists(lno, codes, nlist, first_vid=i0, lists=lists)
            i0 += n
        ix = PR.Index(cc, pq, lists, raw=base)
        assert g.ivfpq_table().tobytes() == ix.T2.tobytes()
        for l in range(nlist):
            ids, cds = g.get_list(l)
            assert np.array_equal(ids, lists[l][0]) and cds.tobytes() == lists[l][1].tobytes(), "list %d" % l
        deleted = rng.choice(N, int(rng.integers(0, N // 4 + 1)), replace=False)
        if deleted.size:
            g.bitmap_set(deleted)
        for _ in range(4):
            nq = int(rng.choice([1, 3, 19, 20, 64, 300]))
            q = np.concatenate([base[rng.integers(0, N, nq // 2)], PR.clustered(nq - nq // 2, d, seed + 50, integer=integer)])
            k = int(rng.choice([1, 5, 10, 33]))
            R = int(rng.choice([1, 7, 40, 100, 300]))
            P = int(rng.integers(1, nlist + 1))
            l2 = bool(rng.integers(0, 2))
            has_rank = bool(rng.integers(0, 2))
            lo, hi = -3e38, 3e38
            ranges = kw_ranges = None
            if rng.integers(0, 2):
                docs = rng.choice(N, int(rng.integers(1, N)), replace=False)
                not_in = bool(rng.integers(0, 2))
                ranges, kw_ranges = [(docs, not_in)], [api.make_range_filter(docs, b_not_in=not_in)]
            filt = PR.Filter(deleted=deleted if deleted.size else None, ranges=ranges)
            args = api.SearchArgs(metric=api.METRIC_L2 if l2 else api.METRIC_IP, nprobe=P, recall_num=R, has_rank=has_rank,
                                  min_score=lo, max_score=hi, range_filters=kw_ranges)
            Dg, Ig = g.ivfpq_search(q, k, args)
            sg = g.last_stages(nq, P, max(R, k))
            D, I, st = ix.search(q, k, P, recall_num=R, has_rank=has_rank, l2=l2, min_score=lo, max_score=hi, filt=filt)
            compare_search_exact(D, I, st, Dg, Ig, sg)
        assert g.ties_not_honoured() == 0
    finally:
        g.close()
