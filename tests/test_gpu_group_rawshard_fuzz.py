"""GPU: seeded random group configurations with raw vectors sharded with their lists -- members, owner weights, metric,
batch sizes -- interleaving add, update, delete and search; strictly against the single handle fed the same calls
(tests/test_gpu_group.py's yardstick), and every row exactly once at the member that lists its vector after every step.
Seeds: GAMMA_RAWSHARD_FUZZ_SEEDS (comma-separated; default a small fixed set)."""
import os

import numpy as np
import pytest

from gamma_amd import api, synth
from tests.lloyd import train_ivfpq
from tests.parity import compare_exact

pytestmark = pytest.mark.gpu

SEEDS = [int(s) for s in os.environ.get("GAMMA_RAWSHARD_FUZZ_SEEDS", "1,2,3,4").split(",") if s.strip()]
WIDE = dict(min_score=-3e38, max_score=3e38)


@pytest.mark.parametrize("seed", SEEDS)
def test_rawshard_group_fuzz(seed):
    rng = np.random.default_rng(1000 + seed)
    W = int(rng.choice([1, 2, 3, 4]))
    M = int(rng.choice([4, 8, 16]))
    d = M * int(rng.choice([2, 4, 8]))
    nlist = int(rng.choice([8, 24, 64]))
    N = int(rng.integers(1500, 6000))
    index_metric = api.METRIC_L2 if rng.integers(0, 2) else api.METRIC_IP
    pool = synth.sift_like(N + 2000, d=d, seed=seed)          # vectors to add, and a reserve to update from
    cc, pq = train_ivfpq(pool[:N], nlist, M, niter=4, pq_niter=3, seed=seed)
    one = api.GammaHip(0)
    grp = api.GammaHipGroup([0] * W)
    try:
        for g in [one] + grp.members:
            g.ivfpq_init(d, nlist, M, 8, index_metric, int(rng.integers(1, 600)))
            g.ivfpq_set_trained(cc, pq, None)
            g.raw_init(d)
        grp.set_raw_placement(True)
        grp.set_owners(rng.integers(0, 100, size=nlist).astype(np.int64) if rng.integers(0, 2) else None)
        added = 0
        dead = np.zeros(0, np.int64)

        def check_rows():
            if added == 0:
                return
            vids = np.arange(added, dtype=np.int64)
            held = np.stack([m.has_vid(vids) for m in grp.members])
            alive = ~np.isin(vids, dead)
            assert (held[:, alive].sum(axis=0) == 1).all()       # (a deleted vector leaves its list at the next compaction)
            stats = [m.raw_sparse_stats() for m in grp.members]
            assert sum(st["live"] for st in stats) == added        # a row per vector ever added: moved, never doubled or lost
            for i, st in enumerate(stats):
                assert st["live"] >= int(held[i].sum()) and st["live"] + st["free"] == st["slots"], (i, st)

        def search():
            nq = int(rng.choice([1, 3, 19, 20, 64, 300]))
            q = np.concatenate([pool[rng.integers(0, max(1, added), nq // 2)], synth.sift_like(nq - nq // 2, d=d, seed=seed + 50)])
            k = int(rng.choice([1, 5, 10, 33]))
            R = int(rng.choice([1, 7, 40, 100, 300]))
            P = int(rng.integers(1, nlist + 1))
            kw = dict(WIDE)
            if rng.integers(0, 3) == 0 and added:
                docs = rng.choice(added, int(rng.integers(1, added + 1)), replace=False)
                kw["range_filters"] = [api.make_range_filter(docs, b_not_in=bool(rng.integers(0, 2)))]
            a = api.SearchArgs(metric=api.METRIC_L2 if rng.integers(0, 2) else api.METRIC_IP, nprobe=P, recall_num=R,
                               has_rank=bool(rng.integers(0, 3)), **kw)
            D, I = one.ivfpq_search(q, k, a)
            Dg, Ig = grp.ivfpq_search(q, k, a)
            compare_exact(D, I, Dg, Ig)

        for step in range(14):
            op = rng.choice(["add", "add", "update", "delete", "search", "search"]) if added else "add"
            if op == "add" and added < N:
                n = int(min(N - added, rng.choice([5, 19, 20, 333, 1500])))
                one.raw_append(pool[added:added + n])
                one.add(pool[added:added + n], added)
                grp.add(pool[added:added + n], added)
                added += n
            elif op == "update":
                n = int(rng.choice([1, 8, 200]))
                vids = rng.integers(0, added + 3, size=n).astype(np.int64)      # repeats and vids never added
                vecs = pool[rng.integers(0, len(pool), size=n)].copy()
                one.update_batch(vids, vecs)
                for v, x in zip(vids, vecs):
                    if v < added:
                        one.raw_update(int(v), x)
                grp.update(vids, vecs)
            elif op == "delete":
                new = rng.choice(added, int(rng.integers(1, max(2, added // 5))), replace=False).astype(np.int64)
                dead = np.union1d(dead, new)
                for g in [one] + grp.members:
                    g.bitmap_set(new)
                one.delete(new)
                grp.delete(new)
                one.compact_if_need()
                grp.compact_if_need()
            else:
                search()
            check_rows()
        search()
        for l in range(nlist):
            ia, ca = grp.get_list(l, M)
            ib, cb = one.get_list(l)
            assert np.array_equal(ia, ib) and np.array_equal(ca, cb), l
    finally:
        grp.close()
        one.close()
