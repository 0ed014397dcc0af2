"""GPU: the HIPIVFPQ plugin with "nsubvector": 96 (a wide index, gamma_hip_ivfpq_wide_init), driven like VectorManager drives a
model -- Indexing, Add, Search, Delete, Dump / Load -- against the CPU oracle."""
import numpy as np
import pytest

from gamma_amd import _lib, plugin, synth
from oracle import binding as B
from tests.parity import compare_exact

pytestmark = pytest.mark.gpu
D_, NLIST, M_, N_ = 192, 8, 96, 4000
PARAM = '{"ncentroids": %d, "nsubvector": %d, "nprobe": 4, "metric_type": "L2"}' % (NLIST, M_)
SEARCH = '{"metric_type": "L2", "recall_num": 50, "nprobe": 4}'


def test_plugin_wide_indexing_add_search_delete_dump_load(tmp_path):
    base = synth.sift_like(N_, d=D_, seed=21)
    q = synth.sift_like(40, d=D_, seed=22)
    m = plugin.PluginModel("HIPIVFPQ", D_, PARAM, indexing_size=N_)
    m2 = plugin.PluginModel("HIPIVFPQ", D_, PARAM, indexing_size=N_)
    m64 = plugin.PluginModel("HIPIVFPQ", D_, PARAM.replace("96", "64"), indexing_size=N_)
    try:
        m.store(base)
        assert m.indexing() == 0
        cc, pq = m.trained_state(NLIST, M_)
        # the training set is the first min(indexing_size, 256 * nlist) vectors (gamma_index_ivfpq.cc:280-301)
        rc, rp = B.ivfpq_train(base[:256 * NLIST], NLIST, M_)
        assert cc.tobytes() == rc.tobytes() and pq.tobytes() == rp.tobytes()
        assert m.add(base)
        o = B.OracleIVFPQ(D_, NLIST, M_, 8, B.METRIC_L2)
        o.set_trained(cc, pq, None)
        B.lib().go_set_assign_mode(-1)
        assert o.add(base)
        o.set_raw(base)
        ctx = dict(min_score=-3e38, max_score=3e38)
        for has_rank in (True, False):
            D, I = o.search(q, 10, 4, recall_num=50, has_rank=has_rank, metric=B.METRIC_L2, ctx=B.make_ctx(**ctx))
            compare_exact(D, I, *m.search(q, 10, SEARCH, has_rank=has_rank))
        # Dump / Load: the IwPQ layout with code_size = M; a model of another nsubvector rejects the file
        D1, I1 = m.search(q, 10, SEARCH)
        assert m.dump(str(tmp_path)) == 0
        m2.store(base)
        assert m2.load(str(tmp_path)) == N_
        D2, I2 = m2.search(q, 10, SEARCH)
        assert D1.tobytes() == D2.tobytes() and np.array_equal(I1, I2)
        m64.store(base)
        assert m64.load(str(tmp_path)) < 0
        # Delete
        dead = np.unique(I1[:, 0])
        dead = dead[dead >= 0]
        assert m.delete(dead) == 0
        bm = np.zeros((N_ + 7) // 8, np.uint8)
        np.bitwise_or.at(bm, dead >> 3, (1 << (dead & 7)).astype(np.uint8))
        D, I = o.search(q, 10, 4, recall_num=50, has_rank=True, metric=B.METRIC_L2, ctx=B.make_ctx(docids_bitmap=bm, **ctx))
        compare_exact(D, I, *m.search(q, 10, SEARCH))
        assert not np.isin(I, dead).any()
    finally:
        B.lib().go_set_assign_mode(0)
        for x in (m, m2, m64):
            x.close()


@pytest.mark.parametrize("M,extra", [(96, '"devices": "0,0"'), (96, '"opq": {"nsubvector": 96}'), (192, '"nbits_per_idx": 4')])
def test_plugin_wide_rejected_key_combinations(M, extra):
    with pytest.raises(_lib.GammaHipError):
        plugin.PluginModel("HIPIVFPQ", 192, '{"ncentroids": 8, "nsubvector": %d, "metric_type": "L2", %s}' % (M, extra))
