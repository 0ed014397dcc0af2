"""CPU: the inputs of the wide-PQ edge and fuzz tests are what those tests claim (tests/pqwide_recipes.py), by the oracle alone.
A GPU test that compares empty rows, a "persistent loop" case in which no workgroup starts a second unit or a "chunked" call
of one chunk would pass and prove nothing."""
import os

import numpy as np
import pytest

from oracle import binding as B
from tests import pqwide_recipes as R


@pytest.mark.parametrize("M", R.EDGE_M)
def test_edge_lists_and_rows_that_still_hold_k_results(M):
    st = R.edge_state(M)
    o = st["oracle"]
    assert R.list_lens(o, st["nlist"]) == [0, 1, 255, 256, 257, 511, 512, 513, 1025, 0, 64, 63]
    # nprobe 12: every query probes both empty lists and the one-code list; nprobe 1: some query probes an empty list, some
    # the one-code list, and every length from 255 on is some query's only list
    _, _, s12 = R.oracle_search(o, st["q"], dict(k=1, P=12, R=1, metric=B.METRIC_L2, has_rank=True))
    assert all(set(row.tolist()) == set(range(12)) for row in s12["coarse_idx"])
    _, _, s1 = R.oracle_search(o, st["q"], dict(k=1, P=1, R=1, metric=B.METRIC_L2, has_rank=True))
    first = set(s1["coarse_idx"][:, 0].tolist())
    assert first & {0, 9} and 1 in first and {2, 3, 4, 5, 6, 7, 8} <= first
    # the 1000-query inner-product call: two probes per workgroup, and segments of an empty list and a one-tile list in both
    # orders (the sums stay in registers past a skipped probe)
    big = R.EDGE_BIG_CALL
    assert R.scan_group_size(big["nq"], big["P"]) == 2 and R.scan_group_size(64, 12) == 1 and R.scan_group_size(2048, 4) == 2
    _, _, sb = R.oracle_search(o, st["q_big"], big)
    seg = np.array(R.EDGE_LENS)[sb["coarse_idx"]].reshape(-1, 2)
    assert ((seg[:, 0] == 0) & (seg[:, 1] > 0) & (seg[:, 1] <= 512)).any() and ((seg[:, 1] == 0) & (seg[:, 0] > 0) & (seg[:, 0] <= 512)).any()
    for variant in R.EDGE_VARIANTS[1:]:
        for call in R.edge_calls():
            q = st["q"][:call["nq"]]
            filt = R.edge_filter(st, variant, call)
            _, I, _ = R.oracle_search(o, q, call, filt)
            assert 4 * R.full_rows(I) >= 3 * len(q), (variant, call, R.full_rows(I))
            if variant == "window":   # ... and the window took something away
                _, I0, _ = R.oracle_search(o, q, call)
                assert call["nq"] < 64 or not np.array_equal(I, I0), call


def test_units_of_the_list_major_case_exceed_twice_the_grid():
    case, q = R.units_case()
    o = case["oracle"]
    for metric in (B.METRIC_L2, B.METRIC_IP):
        _, _, st = R.oracle_search(o, q, dict(k=10, P=4, R=50, metric=metric, has_rank=True))
        assert R.lm_units(R.list_lens(o, 8), st["coarse_idx"]) > 2 * R.LM_GRID


def test_lm_units_counts_slabs_times_tiles():
    # list 0: 257 codes (2 slabs) x 9 pairs (2 tiles); list 1: empty; list 2: 256 codes (1 slab) x 8 pairs (1 tile); list 3: nobody
    probes = np.array([[0, 2]] * 8 + [[0, 1]])
    assert R.lm_units([257, 0, 256, 100], probes) == 2 * 2 + 1


def test_the_budget_of_the_chunked_case_cuts_300_queries_into_ragged_chunks():
    case, base, q = R.ties_case()
    o = R.ties_oracle(case, base)
    lens = R.list_lens(o, 8)
    for metric in (B.METRIC_L2, B.METRIC_IP):
        _, _, st = R.oracle_search(o, q, dict(k=10, P=4, R=10, metric=metric, has_rank=True))
        for limited in (True, False):
            chunk = R.scan_chunk(R.ties_budget(lens, 4), lens, st["coarse_idx"], 96, limited)
            assert -(-300 // chunk) >= 3 and 300 % chunk != 0, chunk
    assert R.scan_chunk(R.BIG_BUDGET, lens, st["coarse_idx"], 96) == 300


def test_scan_chunk_restates_the_two_sizings():
    probes = np.array([[0, 1], [1, 2], [2, 2]])
    lens = [100, 10, 30]
    assert R.scan_chunk(1 << 30, lens, probes, 96) == 3                    # all of the call
    assert R.scan_chunk(2 * 2 * 100 * 4, lens, probes, 96) == 3            # 2 by the longest list, 3 by the longest row (112)
    assert R.scan_chunk(2 * 100 * 4, lens, probes, 96) == 1
    assert R.scan_chunk(1 << 40, lens, np.zeros((20000, 1), np.int64), 256) == 4096   # 1 GB of tables of 256 KB


def test_default_fuzz_seeds_cover_what_the_fuzz_claims():
    assert R.FUZZ_SEEDS == R.FUZZ_DEFAULT_SEEDS or "GAMMA_PQWIDE_FUZZ_SEEDS" in os.environ
    plans = [R.fuzz_plan(s) for s in R.FUZZ_DEFAULT_SEEDS]
    assert len(plans) == 8
    assert any(p["M"] % 32 == 0 for p in plans) and any(p["M"] % 2 == 1 for p in plans)
    assert any(p["ip_index"] for p in plans) and any(not p["ip_index"] for p in plans)
    assert any(p["kind"] != "sift" for p in plans)
    assert any(p["kind"] == "sift" and not p["ip_index"] for p in plans) and any(p["kind"] == "sift" and p["ip_index"] for p in plans)
    assert any(s["R"] < s["k"] for p in plans for s in p["searches"])
    assert any(s["reduced"] for p in plans for s in p["searches"]) and any(s["ranged"] for p in plans for s in p["searches"])
    assert {50, 1000} == {p["bucket"] for p in plans}
    probed_empty, compacted, grown, ip_balanced = 0, [], 0, 0
    for p in plans:
        dt = R.fuzz_data(p)
        o, bm = R.fuzz_oracle(dt)
        assert len(dt["dead"]) <= p["N"] // 4 and len(set(dt["dead"].tolist())) == len(dt["dead"])
        lens, before = np.array(R.list_lens(o, p["nlist"])), np.array(dt["lens_before_compaction"])
        # a compaction that rewrites nothing proves nothing: a list of 20 codes and more has to shrink
        if ((lens < before) & (before >= 20)).any():
            assert p["compact"]
            compacted.append(p["bucket"])
        else:
            assert not p["compact"], "seed %d: CompactIfNeed rewrote no list" % p["seed"]
        grown += int(p["bucket"] == 50 and before.max() > 50)
        ip_balanced += int(p["ip_index"] and (lens > 100).sum() >= 3)
        for i, s in enumerate(p["searches"]):
            _, _, st = R.oracle_search(o, dt["queries"][i], s, R.fuzz_filter(dt, i, bm))
            probed_empty += int((lens[st["coarse_idx"]] == 0).any())
    assert probed_empty >= 1 and grown >= 1 and ip_balanced >= 1
    assert 50 in compacted and 1000 in compacted, compacted   # lists that grew from a small bucket are compacted too


def test_the_inner_product_edge_index_has_balanced_lists():
    from tests.pqwide_recipes import ip_case
    for M in (65, 128):
        c = ip_case(M)
        lens = np.array(R.list_lens(c["oracle"], c["nlist"]))
        assert (lens > 100).sum() >= 3 and lens.max() < 0.6 * lens.sum(), lens
