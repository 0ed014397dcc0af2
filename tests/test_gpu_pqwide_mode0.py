"""GPU: wide 8-bit IVFPQ handles (65 .. 256 sub-quantizers) in L2 TABLE MODE 0 -- gamma_hip_ivfpq_wide_set_table_mode0, the scan of
pqwide_res.hip -- against the CPU oracle in mode 0 (faiss:IndexIVFPQ.cpp:441-449, index/impl/gamma_index_ivfpq.h:239-245),
strictly: compare_search_exact, exact ties on, no query excluded.  The oracle's mode-0 distances differ in their bits from its
mode-1 distances, so a scan with the precomputed table's arithmetic fails here."""
import numpy as np
import pytest

from gamma_amd import api, synth
from oracle import binding as B
from tests import fixtures
from tests.parity import compare_search_exact
from tests.test_gpu_mode0 import table_limit   # the oracle's and the device library's limit together, restored afterwards

pytestmark = pytest.mark.gpu
WIDE = dict(min_score=-3e38, max_score=3e38)
# (d, M): dsub 1 with an odd M, a last slice of one and rows aligned to their element only | dsub 2, whole slices | dsub 4 | 8 |
# 12 | 3 (generic row with a tail) | 16 (generic AVX row) | eight slices, the M limit
SHAPES = [(65, 65), (192, 96), (260, 65), (520, 65), (780, 65), (195, 65), (1040, 65), (256, 256)]


def _handle(case, o, base=None, mode0=True):
    """tests/test_gpu_pqwide.py's handle, with the switch; the caller holds the limit"""
    g = api.GammaHip(0)
    g.ivfpq_wide_init(case["d"], case["nlist"], case["M"], case["metric"], table_mode0=mode0)
    g.ivfpq_set_trained(case["cc"], case["pq"], None)
    g.raw_init(case["d"])
    g.raw_append(case["base"] if base is None else base)
    lists = [(l,) + o.get_list(l) for l in range(case["nlist"])]
    lists = [t for t in lists if len(t[1])]
    g.add_keys_batch([t[0] for t in lists], [len(t[1]) for t in lists], np.concatenate([t[1] for t in lists]),
                     np.concatenate([t[2] for t in lists]))
    return g


def _mode0(case, base=None):
    """(oracle, handle) of the case's trained state, both created under a limit one byte below the table"""
    base = case["base"] if base is None else base
    with table_limit(case["nlist"] * case["M"] * 1024 - 1):
        o = B.OracleIVFPQ(case["d"], case["nlist"], case["M"], 8, B.METRIC_L2)
        o.set_trained(case["cc"], case["pq"], None)
        assert o.use_precomputed_table() == 0
        B.lib().go_set_assign_mode(0)
        assert o.add(base)
        o.set_raw(base)
        g = _handle(case, o, base)
    assert g.use_precomputed_table() == 0
    return o, g


def _case(d, M):   # tests/test_gpu_pqwide.py's recipe (cached): lists longer than one tile and shorter than 256
    return fixtures.trained_case(d, nlist=8, M=M, N=5000, nq=64)


def _check(o, g, q, k, P, R, has_rank=True, metric=B.METRIC_L2, bitmap=None, ranges=None, not_in=False):
    rf_o = [B.make_range_filter(r, b_not_in=not_in) for r in ranges] if ranges else None
    rf_g = [api.make_range_filter(r, b_not_in=not_in) for r in ranges] if ranges else None
    D, I, st = o.search(q, k, P, recall_num=R, has_rank=has_rank, metric=metric,
                        ctx=B.make_ctx(docids_bitmap=bitmap, range_filters=rf_o, **WIDE), want_stages=True)
    Dg, Ig = g.ivfpq_search(q, k, api.SearchArgs(metric=metric, nprobe=P, recall_num=R, has_rank=has_rank, range_filters=rf_g, **WIDE))
    compare_search_exact(D, I, st, Dg, Ig, g.last_stages(len(q), P, max(R, k)))


@pytest.fixture(scope="module")
def c96():
    case = _case(192, 96)
    o, g = _mode0(case)
    yield case, o, g
    g.close()


@pytest.mark.parametrize("d,M", SHAPES)
def test_mode0_search_and_answers(d, M):
    case = _case(d, M)
    o, g = _mode0(case)
    g1 = _handle(case, o, mode0=False)   # the default limit: mode 1, with its table
    try:
        for has_rank in (True, False):
            _check(o, g, case["q"], 10, 4, 50, has_rank)
        _check(o, g, case["q"], 10, 4, 50, metric=B.METRIC_IP)
        assert g.ties_not_honoured() == 0
        assert g.use_precomputed_table() == 0 and g1.use_precomputed_table() == 1
        with pytest.raises(api.GammaHipError, match="table mode 0"):
            g.ivfpq_table()
        assert g1.total_mem_bytes() - g.total_mem_bytes() >= 8 * M * 1024   # no table (and no code sums) on the device
    finally:
        g.close()
        g1.close()


@pytest.mark.parametrize("nq", [1, 3, 2048])
def test_batch_sizes(c96, nq):
    _, o, g = c96
    _check(o, g, synth.sift_like(nq, d=192, seed=700 + nq), 10, 4, 50)


@pytest.mark.parametrize("not_in", [False, True])
def test_deleted_documents_and_a_range_filter(c96, not_in):
    case, o, g = c96
    rng = np.random.default_rng(5)
    deleted = rng.choice(5000, 1000, replace=False)   # 20 %
    bm = np.zeros((5000 + 7) // 8, np.uint8)
    np.bitwise_or.at(bm, deleted >> 3, (1 << (deleted & 7)).astype(np.uint8))
    g.bitmap_set(deleted)
    try:
        _check(o, g, case["q"], 10, 4, 50, bitmap=bm, ranges=[rng.choice(5000, 2500, replace=False)], not_in=not_in)
    finally:
        g.bitmap_set(deleted, 0)


def test_exact_ties_at_the_recall_cut():
    case = _case(192, 96)
    base = synth.sift_like(2200, d=192, seed=77)
    base = np.concatenate([base, np.repeat(base[:200], 3, axis=0)])   # 200 rows four times each: equal codes in one list
    o, g = _mode0(case, base)
    try:
        for has_rank in (True, False):
            _check(o, g, base[:64] + np.float32(0.25), 10, 4, 10, has_rank)
        assert g.ties_not_honoured() == 0
    finally:
        g.close()


def test_the_switch(c96):
    case, _, g0 = c96
    g = api.GammaHip(0)
    try:
        assert g.ivfpq_wide_table_mode0() == 0
        with table_limit(8 * 96 * 1024 - 1):   # off plus a lowered limit: refused as ever
            with pytest.raises(api.GammaHipError, match="precomputed_table_max_bytes"):
                g.ivfpq_wide_init(192, 8, 96)
    finally:
        g.close()
    # on plus the default limit: mode 1, the answers of a handle made without the switch byte for byte
    o1 = case["oracle"]
    ga, gb = _handle(case, o1, mode0=True), _handle(case, o1, mode0=False)
    try:
        assert ga.ivfpq_wide_table_mode0() == 1 and ga.use_precomputed_table() == 1
        args = api.SearchArgs(metric=api.METRIC_L2, nprobe=4, recall_num=50, has_rank=True, **WIDE)
        (Da, Ia), (Db, Ib) = ga.ivfpq_search(case["q"], 10, args), gb.ivfpq_search(case["q"], 10, args)
        assert Da.tobytes() == Db.tobytes() and Ia.tobytes() == Ib.tobytes()
        with pytest.raises(api.GammaHipError, match="before"):   # the table mode is fixed at the init
            ga.ivfpq_wide_set_table_mode0(False)
    finally:
        ga.close()
        gb.close()
    with pytest.raises(api.GammaHipError, match="table mode 0"):   # the list-major scan reads the table
        g0.ivfpq_wide_set_lm_scan(True)
