"""GPU: the list-major scan of a wide IVFPQ handle (gamma_hip_ivfpq_wide_set_lm_scan, k_ivfpq_scan_wide_lm of pqwide_lm.hip) against the
CPU oracle through compare_search_exact (exact ties on, no query excluded), and against the same handle with the switch off.
Lists of ~625 codes: several slabs of 256 with a partial last one; 64 queries x nprobe 4 over 8 lists: ~32 pairs per list,
several tiles of 8 with a partial one."""
import numpy as np
import pytest

from gamma_amd import api, synth
from oracle import binding as B
from tests.test_gpu_pqwide import _case, _check, _handle

pytestmark = pytest.mark.gpu
METRICS = (B.METRIC_L2, B.METRIC_IP)


@pytest.fixture(scope="module")
def c96():
    case = _case(192, 96)
    g = _handle(case)
    g.ivfpq_wide_set_lm_scan(1)
    yield case, g
    g.close()


def _answer(g, q, metric, has_rank):
    a = api.SearchArgs(metric=metric, nprobe=4, recall_num=50, has_rank=has_rank, min_score=-3e38, max_score=3e38)
    D, I = g.ivfpq_search(q, 10, a)
    st = g.last_stages(len(q), 4, 50)
    return D.tobytes(), I.tobytes(), {k: np.asarray(v).tobytes() for k, v in st.items()}


@pytest.mark.parametrize("d,M", [(192, 96), (256, 128), (512, 256)])   # 3, 4 and 8 slices
def test_shapes_against_the_oracle_and_the_pair_scan(d, M):
    case = _case(d, M)
    ms, qt, lds = api.ivfpq_wide_lm_shape(M)
    assert ms == 32 and lds == 2 * ms * 1024 and qt >= 1
    g = _handle(case)
    try:
        assert g.ivfpq_wide_lm_scan() == 0
        off = [_answer(g, case["q"], m, r) for m in METRICS for r in (True, False)]
        assert g.ivfpq_wide_lm_stats() == (0, -1, 0)
        g.ivfpq_wide_set_lm_scan(1)
        assert g.ivfpq_wide_lm_scan() == 1
        for metric in METRICS:
            for has_rank in (True, False):
                _check(case["oracle"], g, case["q"], 10, 4, 50, has_rank, metric)
        assert g.ivfpq_wide_lm_stats() == (4, -1, 4 * 64 * 4)
        assert [_answer(g, case["q"], m, r) for m in METRICS for r in (True, False)] == off
        assert g.ties_not_honoured() == 0
    finally:
        g.close()


@pytest.mark.parametrize("nq", [1, 3, 300])   # tiles of fewer than 8 pairs and lists nobody probes | more than one tile per list
def test_batch_sizes(c96, nq):
    case, g = c96
    q = synth.sift_like(nq, d=192, seed=700 + nq)
    calls = g.ivfpq_wide_lm_stats()[0]
    for metric in METRICS:
        _check(case["oracle"], g, q, 10, 4, 50, metric=metric)
    assert g.ivfpq_wide_lm_stats()[0] == calls + 2


@pytest.mark.parametrize("not_in", [False, True])
def test_deleted_documents_and_a_range_filter(c96, not_in):
    case, g = c96
    rng = np.random.default_rng(5)
    deleted = rng.choice(5000, 1000, replace=False)   # 20 %
    bm = np.zeros((5000 + 7) // 8, np.uint8)
    np.bitwise_or.at(bm, deleted >> 3, (1 << (deleted & 7)).astype(np.uint8))
    g.bitmap_set(deleted)
    calls = g.ivfpq_wide_lm_stats()[0]
    try:
        _check(case["oracle"], g, case["q"], 10, 4, 50, bitmap=bm, ranges=[rng.choice(5000, 2500, replace=False)], not_in=not_in)
    finally:
        g.bitmap_set(deleted, 0)
    assert g.ivfpq_wide_lm_stats()[0] == calls + 1


def test_an_M_the_kernel_does_not_serve_and_a_handle_that_is_not_wide():
    assert api.ivfpq_wide_lm_shape(65)[0] == 0
    case = _case(130, 65)
    g, plain = _handle(case), api.GammaHip(0)
    try:
        g.ivfpq_wide_set_lm_scan(1)
        _check(case["oracle"], g, case["q"], 10, 4, 50)
        assert g.ivfpq_wide_lm_stats() == (0, -1, 0)
        plain.ivfpq_init(32, 8, 8, 8, B.METRIC_L2)
        with pytest.raises(api.GammaHipError, match="wide handle"):
            plain.ivfpq_wide_set_lm_scan(1)
        assert plain.ivfpq_wide_lm_scan() == 0
    finally:
        g.close()
        plain.close()
