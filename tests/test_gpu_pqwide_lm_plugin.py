"""GPU: the HIPIVFPQ plugin with "nsubvector": 96, "pqwide_lm_scan": 1 (a wide index scanned list-major) against the CPU oracle;
the key on a model that is not wide makes Init fail."""
import pytest

from gamma_amd import _lib, plugin, synth
from oracle import binding as B
from tests.parity import compare_exact

pytestmark = pytest.mark.gpu
D_, NLIST, M_, N_ = 192, 8, 96, 4000
PARAM = '{"ncentroids": %d, "nsubvector": %d, "nprobe": 4, "metric_type": "L2", "pqwide_lm_scan": 1}' % (NLIST, M_)
SEARCH = '{"metric_type": "L2", "recall_num": 50, "nprobe": 4}'


def test_plugin_wide_lm_scan_answers_as_the_oracle():
    base = synth.sift_like(N_, d=D_, seed=21)
    q = synth.sift_like(40, d=D_, seed=22)
    m = plugin.PluginModel("HIPIVFPQ", D_, PARAM, indexing_size=N_)
    try:
        m.store(base)
        assert m.indexing() == 0 and m.add(base)
        cc, pq = m.trained_state(NLIST, M_)
        o = B.OracleIVFPQ(D_, NLIST, M_, 8, B.METRIC_L2)
        o.set_trained(cc, pq, None)
        B.lib().go_set_assign_mode(-1)
        assert o.add(base)
        o.set_raw(base)
        assert m.ivfpq_wide_lm_stats() == (0, 0)
        for has_rank in (True, False):
            D, I = o.search(q, 10, 4, recall_num=50, has_rank=has_rank, metric=B.METRIC_L2,
                            ctx=B.make_ctx(min_score=-3e38, max_score=3e38))
            compare_exact(D, I, *m.search(q, 10, SEARCH, has_rank=has_rank))
        assert m.ivfpq_wide_lm_stats() == (2, 2 * len(q) * 4)
    finally:
        B.lib().go_set_assign_mode(0)
        m.close()


def test_plugin_rejects_the_key_on_a_model_that_is_not_wide():
    with pytest.raises(_lib.GammaHipError):
        plugin.PluginModel("HIPIVFPQ", D_, PARAM.replace("96", "16"))
