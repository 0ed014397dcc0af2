"""GPU: seeded random wide IVFPQ configurations (65 .. 256 sub-quantizers) -- shapes, index metric, SIFT-shaped or small-grid data
(most queries tie at the recall cut), lists that grow from a small bucket, Add in batches on both sides of the 20-vector rule,
Delete, Update, CompactIfNeed, then searches with k and recall_num on both sides of each other, nprobe 1 .. nlist, either
request metric, range filters, now and then a workspace budget that cuts the call into sub-batches -- strictly against the CPU
oracle (compare_search_exact, no query excluded).  The pair scan is always checked, the list-major scan where the kernel serves
M, table mode 0 on an L2 index; every handle goes through the same writes and searches.
Seeds: GAMMA_PQWIDE_FUZZ_SEEDS (comma-separated; default pqwide_recipes.FUZZ_DEFAULT_SEEDS, whose coverage tests/test_pqwide_recipes_cpu.py asserts)."""
import numpy as np
import pytest

from oracle import binding as B
from tests import pqwide_recipes as R
from tests.parity import compare_exact
from tests.test_gpu_mode0 import table_limit
from tests.test_gpu_pqwide_edges import check, close_all, device_search, lm_serves, new_handle

pytestmark = pytest.mark.gpu


def _same_lists(g, o, nlist, what):
    for l in range(nlist):
        (ig, cg), (io, co) = g.get_list(l), o.get_list(l)
        assert np.array_equal(ig, io) and cg.tobytes() == co.tobytes(), "%s: list %d" % (what, l)
        assert g.list_capacity(l) == o.list_capacity(l), "%s: capacity of list %d" % (what, l)


def _write(g, dt):
    """the plan's Add path on a handle (tests/pqwide_recipes.py fuzz_oracle_add on the oracle's side)"""
    N = dt["N"]
    g.raw_init(dt["d"])
    g.raw_append(dt["base"])
    g.bitmap_upload(np.zeros((N + 64) // 8 + 1, dtype=np.uint8), N + 64)
    at = 0
    for n in dt["batches"]:
        g.add(dt["base"][at:at + n], at)
        at += n


def _edit(g, dt):
    if len(dt["dead"]):
        g.bitmap_set(dt["dead"], 1)
        g.delete(dt["dead"])
    for newl, vid, code in dt["updates"]:
        g.update(newl, vid, code)
    if dt["compact"]:
        g.compact_if_need()


@pytest.mark.parametrize("seed", R.FUZZ_SEEDS)
def test_pqwide_fuzz(seed):
    dt = R.fuzz_data(R.fuzz_plan(seed))
    M, nlist = dt["M"], dt["nlist"]
    pairs = []   # (handle, oracle of its L2 searches, that oracle's bitmap, name)
    try:
        B.lib().go_set_assign_mode(-1)   # faiss's rule on both sides: fewer than 20 vectors exact, else the GEMM form
        o1 = B.OracleIVFPQ(dt["d"], nlist, M, 8, dt["metric"], bucket_init_size=dt["bucket"])
        bm1 = R.fuzz_oracle_add(o1, dt)
        pairs.append((new_handle(dt, bucket=dt["bucket"]), o1, bm1, "pair"))
        if lm_serves(M):
            g = new_handle(dt, bucket=dt["bucket"])
            g.ivfpq_wide_set_lm_scan(1)
            pairs.append((g, o1, bm1, "list-major"))
        if not dt["ip_index"]:
            with table_limit(nlist * M * 1024 - 1):
                o0 = B.OracleIVFPQ(dt["d"], nlist, M, 8, dt["metric"], bucket_init_size=dt["bucket"])
                bm0 = R.fuzz_oracle_add(o0, dt)
                assert o0.use_precomputed_table() == 0
                pairs.append((new_handle(dt, mode0=True, bucket=dt["bucket"]), o0, bm0, "mode 0"))
            assert pairs[-1][0].use_precomputed_table() == 0
        for g, o, _, name in pairs:
            _write(g, dt)
            _same_lists(g, o, nlist, name + " after add")
        B.lib().go_set_assign_mode(0)
        R.fuzz_edits(o1, dt)   # (on a compacting seed the deletes gather in one or two lists, which CompactIfNeed then rewrites)
        R.fuzz_oracle_edit(o1, bm1, dt)
        if not dt["ip_index"]:
            R.fuzz_oracle_edit(o0, bm0, dt)
        for g, o, _, name in pairs:
            _edit(g, dt)
            _same_lists(g, o, nlist, name + " after delete / update / compact")
        for i, call in enumerate(dt["searches"]):
            q = dt["queries"][i]
            want1 = R.oracle_search(o1, q, call, R.fuzz_filter(dt, i, bm1))
            for g, o, bm, name in pairs:
                filt = R.fuzz_filter(dt, i, bm)
                want = want1 if (o is o1 or call["metric"] == B.METRIC_IP) else R.oracle_search(o, q, call, filt)
                whole = check(want, g, q, call, filt)
                if call["reduced"]:   # the same call in sub-batches (the stages kept are the last one's: the answers only)
                    g.set_dist_budget(R.fuzz_budget(call["P"], g.max_list_len()))
                    try:
                        Dg, Ig, _ = device_search(g, q, call, filt)
                    finally:
                        g.set_dist_budget(R.BIG_BUDGET)
                    compare_exact(want[0], want[1], Dg, Ig)
                    assert (Dg.tobytes(), Ig.tobytes()) == whole, (name, i)
        for g, _, _, name in pairs:
            assert g.ties_not_honoured() == 0, name
            if name == "list-major":
                assert g.ivfpq_wide_lm_stats()[0] >= 4
            else:
                assert g.ivfpq_wide_lm_stats() == (0, -1, 0)
    finally:
        B.lib().go_set_assign_mode(0)
        close_all([p[0] for p in pairs])
