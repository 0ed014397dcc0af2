"""GPU: wide 8-bit IVFPQ handles (gamma_hip_ivfpq_wide_init, 65 .. 256 sub-quantizers; the sliced-table scan of pqwide.hip) against
the CPU oracle, strictly: table and codes byte-equal, searches through compare_search_exact (exact ties on, no query excluded)."""
import ctypes as C

import numpy as np
import pytest

from gamma_amd import api, synth
from oracle import binding as B
from tests import fixtures
from tests.parity import compare_search_exact

pytestmark = pytest.mark.gpu
WIDE = dict(min_score=-3e38, max_score=3e38)
SHAPES = [(130, 65), (192, 96), (256, 128), (512, 256)]   # odd M: byte loads, a last slice of one | 3 | 4 | 8 whole slices (the limit)


def _case(d, M):
    return fixtures.trained_case(d, nlist=8, M=M, N=5000, nq=64)


def _handle(case, base=None, oracle=None):
    """fixtures.load_hip for a handle made by ivfpq_wide_init"""
    o = oracle or case["oracle"]
    g = api.GammaHip(0)
    g.ivfpq_wide_init(case["d"], case["nlist"], case["M"], case["metric"])
    g.ivfpq_set_trained(case["cc"], case["pq"], None)
    g.raw_init(case["d"])
    g.raw_append(case["base"] if base is None else base)
    lists = [(l,) + o.get_list(l) for l in range(case["nlist"])]
    lists = [t for t in lists if len(t[1])]
    g.add_keys_batch([t[0] for t in lists], [len(t[1]) for t in lists], np.concatenate([t[1] for t in lists]),
                     np.concatenate([t[2] for t in lists]))
    return g


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
    g = _handle(case)
    yield case, g
    g.close()


@pytest.mark.parametrize("d,M", SHAPES)
def test_table_codes_and_search(d, M):
    case = _case(d, M)
    o = case["oracle"]
    ms, ns, lds, tile = api.ivfpq_wide_shape(M)
    assert ms * (ns - 1) < M <= ms * ns and lds == ms * 1024 <= 65536
    lens = [len(o.get_list(l)[0]) for l in range(8)]
    assert max(lens) > tile, "no list parks its sums in the slab"
    assert M < 96 or min(lens) < 256, "no list shorter than a wave step"
    g = _handle(case)
    try:
        assert g.code_size() == M
        assert g.ivfpq_table().tobytes() == o.table().tobytes(), "precomputed table"
        lno, codes = g.encode(case["base"][:300])
        B.lib().go_set_assign_mode(-1)                 # 300 vectors: the GEMM form on both sides
        rl, rc = o.encode(case["base"][:300])
        B.lib().go_set_assign_mode(0)                  # (as fixtures.trained_case leaves it)
        assert np.array_equal(lno, rl) and codes.tobytes() == rc.tobytes(), "encode"
        for metric, has_rank in ((B.METRIC_L2, True), (B.METRIC_L2, False), (B.METRIC_IP, True), (B.METRIC_IP, False)):
            _check(o, g, case["q"], 10, 4, 50, has_rank, metric)
        assert g.ties_not_honoured() == 0
    finally:
        g.close()


@pytest.mark.parametrize("nq", [1, 3, 64, 2048])
def test_batch_sizes(c96, nq):
    case, g = c96
    q = synth.sift_like(nq, d=192, seed=700 + nq)
    _check(case["oracle"], g, q, 10, 4, 50)
    _check(case["oracle"], g, q, 10, 4, 50, metric=B.METRIC_IP)


@pytest.mark.parametrize("not_in", [False, True])
def test_deleted_documents_and_a_range_filter(c96, not_in):
    case, g = c96
    rng = np.random.default_rng(5)
    deleted = rng.choice(5000, 1000, replace=False)   # 20 %
    bm = np.zeros((5000 + 7) // 8, np.uint8)
    np.bitwise_or.at(bm, deleted >> 3, (1 << (deleted & 7)).astype(np.uint8))
    g.bitmap_set(deleted)
    try:
        _check(case["oracle"], g, case["q"], 10, 4, 50, bitmap=bm, ranges=[rng.choice(5000, 2500, replace=False)], not_in=not_in)
    finally:
        g.bitmap_set(deleted, 0)


def test_exact_ties_at_the_recall_cut(c96):
    case, _ = c96
    base = synth.sift_like(2200, d=192, seed=77)
    base = np.concatenate([base, np.repeat(base[:200], 3, axis=0)])   # 200 rows four times each: equal codes in one list
    o = B.OracleIVFPQ(192, 8, 96, 8, B.METRIC_L2)
    o.set_trained(case["cc"], case["pq"], None)
    B.lib().go_set_assign_mode(0)
    assert o.add(base)
    o.set_raw(base)
    g = _handle(case, base, o)
    try:
        for has_rank in (True, False):
            _check(o, g, base[:64] + np.float32(0.25), 10, 4, 10, has_rank)
        assert g.ties_not_honoured() == 0
    finally:
        g.close()


def test_train_on_a_wide_handle(c96):
    case, g = c96[0], api.GammaHip(0)
    try:
        g.ivfpq_wide_init(192, 8, 96)
        cc, pq = g.ivfpq_train(case["base"], 8, 96)   # fixtures.trained_case trains on these 5000 rows with B.ivfpq_train
        assert cc.tobytes() == case["cc"].tobytes() and pq.tobytes() == case["pq"].tobytes()
    finally:
        g.close()


def test_refusals_say_so(c96):
    gw, g, old = c96[1], api.GammaHip(0), api.get_precomputed_table_max_bytes()
    try:
        with pytest.raises(api.GammaHipError, match="nsubvector > 64 unsupported"):
            g.ivfpq_init(192, 8, 96)
        for d, M in ((128, 64), (257, 257)):
            with pytest.raises(api.GammaHipError, match="65 .. 256"):
                g.ivfpq_wide_init(d, 8, M)
        api.set_precomputed_table_max_bytes(8 * 96 * 256 * 4 - 1)
        with pytest.raises(api.GammaHipError, match="precomputed_table_max_bytes"):
            g.ivfpq_wide_init(192, 8, 96)
    finally:
        api.set_precomputed_table_max_bytes(old)
        g.close()
    import torch
    buf = torch.zeros(1 << 16, dtype=torch.float32, device="cuda:0")
    p = C.c_void_p(buf.data_ptr())
    a = api.SearchArgs(metric=api.METRIC_L2, nprobe=4, recall_num=20, has_rank=False, **WIDE).ref()
    L, h = gw.L, gw.h
    for name, fn in (("search_shard", lambda: L.gamma_hip_ivfpq_search_shard(h, a, 4, p, 10, p, p)),
                     ("set_list_mask", lambda: L.gamma_hip_ivfpq_set_list_mask(h, np.ones(8, np.uint8).ctypes.data_as(C.POINTER(C.c_uint8)))),
                     ("opq_set", lambda: L.gamma_hip_opq_set(h, np.eye(192, dtype=np.float32).ctypes.data_as(C.POINTER(C.c_float))))):
        rc, msg = fn(), L.gamma_hip_last_error(h).decode()
        assert rc == -6 and "wide handle" in msg, (name, rc, msg)   # GAMMA_HIP_EUNSUPPORTED
