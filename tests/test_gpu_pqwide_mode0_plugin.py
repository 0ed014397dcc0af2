"""GPU: the HIPIVFPQ plugin with "nsubvector": 96, "pqwide_table_mode0": 1 created while precomputed_table_max_bytes is below its
table (a wide index in L2 table mode 0) against the CPU oracle in mode 0, through Dump / Load; where the key is rejected."""
import pytest

from gamma_amd import _lib, plugin, synth
from oracle import binding as B
from tests.parity import compare_exact
from tests.test_gpu_mode0 import table_limit

pytestmark = pytest.mark.gpu
D_, NLIST, M_, N_ = 192, 8, 96, 4000
PARAM = '{"ncentroids": %d, "nsubvector": %d, "nprobe": 4, "metric_type": "L2", "pqwide_table_mode0": 1}' % (NLIST, M_)
SEARCH = '{"metric_type": "L2", "recall_num": 50, "nprobe": 4}'


def test_plugin_wide_mode0_answers_as_the_oracle(tmp_path):
    base = synth.sift_like(N_, d=D_, seed=21)
    q = synth.sift_like(40, d=D_, seed=22)
    with table_limit(NLIST * M_ * 1024 - 1):
        with pytest.raises(_lib.GammaHipError):   # without the key: Init fails as ever
            plugin.PluginModel("HIPIVFPQ", D_, PARAM.replace(', "pqwide_table_mode0": 1', ""))
        m = plugin.PluginModel("HIPIVFPQ", D_, PARAM, indexing_size=N_)
        m2 = plugin.PluginModel("HIPIVFPQ", D_, PARAM, indexing_size=N_)
    try:
        m.store(base)
        assert m.indexing() == 0 and m.add(base)
        cc, pq = m.trained_state(NLIST, M_)
        with table_limit(NLIST * M_ * 1024 - 1):
            o = B.OracleIVFPQ(D_, NLIST, M_, 8, B.METRIC_L2)
            o.set_trained(cc, pq, None)
        assert o.use_precomputed_table() == 0
        B.lib().go_set_assign_mode(-1)
        assert o.add(base)
        o.set_raw(base)
        for has_rank in (True, False):
            D, I = o.search(q, 10, 4, recall_num=50, has_rank=has_rank, metric=B.METRIC_L2,
                            ctx=B.make_ctx(min_score=-3e38, max_score=3e38))
            Dg, Ig = m.search(q, 10, SEARCH, has_rank=has_rank)
            compare_exact(D, I, Dg, Ig)
        # Dump / Load into a model created the same way: mode 0 again, the same bytes
        assert m.dump(str(tmp_path)) == 0
        m2.store(base)
        assert m2.load(str(tmp_path)) == N_
        D2, I2 = m2.search(q, 10, SEARCH, has_rank=False)
        assert D2.tobytes() == Dg.tobytes() and I2.tobytes() == Ig.tobytes()
    finally:
        B.lib().go_set_assign_mode(0)
        m.close()
        m2.close()


@pytest.mark.parametrize("param", [PARAM.replace("96", "16"), PARAM.replace('"nprobe"', '"nbits_per_idx": 4, "nprobe"'),
                                   PARAM.replace('"nprobe"', '"pqwide_lm_scan": 1, "nprobe"')])
def test_plugin_rejects_the_key(param):
    """on a model with nsubvector <= 64, with 4-bit codes, and beside the list-major scan (which reads the table)"""
    with pytest.raises(_lib.GammaHipError):
        plugin.PluginModel("HIPIVFPQ", D_, param)
