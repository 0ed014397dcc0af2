"""GPU: HIPIVFPQ with "nbits_per_idx": 4, "pq4_lm_scan": 1 equals the model without the key; the counters show the launches."""
import numpy as np
import pytest

from tests import pq4_ref as PR

pytestmark = pytest.mark.gpu

D_, NLIST, M_, N_ = 32, 16, 8, 4000
PARAM = '{"ncentroids": %d, "nsubvector": %d, "nbits_per_idx": 4, "nprobe": 6, "metric_type": "L2"%%s}' % (NLIST, M_)


def test_plugin_lm_scan_equals_the_model_without_the_key():
    from gamma_amd import plugin
    base = PR.clustered(N_, D_, 3)
    q = PR.clustered(48, D_, 9)
    cc, pq = PR.train(base[:3000], NLIST, M_)
    models = [plugin.PluginModel("HIPIVFPQ", D_, PARAM % extra, indexing_size=3000) for extra in ("", ', "pq4_lm_scan": 1')]
    try:
        for m in models:
            m.store(base)
            assert m.set_trained(cc, pq) == 0 and m.add(base)
        assert models[0].ivfpq4_lm_stats() is None and models[1].ivfpq4_lm_stats() == (0, 0)   # no key: no list-major ops
        for has_rank in (True, False):
            D0, I0 = models[0].search(q, 10, '{"metric_type": "L2", "recall_num": 100, "nprobe": 6}', has_rank=has_rank)
            D1, I1 = models[1].search(q, 10, '{"metric_type": "L2", "recall_num": 100, "nprobe": 6}', has_rank=has_rank)
            assert D0.tobytes() == D1.tobytes() and np.array_equal(I0, I1)
        assert models[1].ivfpq4_lm_stats() == (2, 2 * len(q) * 6)
    finally:
        for m in models:
            m.close()
