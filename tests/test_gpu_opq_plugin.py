"""GPU: the HIPIVFPQ plugin with "opq": {"nsubvector": N}, driven as VectorManager drives a model (store, Indexing, Add in
engine-sized batches, Update, Search, Dump, Load) against the yardstick of tests/opq_ref.py built from the plugin's own
trained state and matrix; the dumped file carries the "LTra" record where the reference writes it."""
import os
import struct

import numpy as np
import pytest

from gamma_amd import _lib
from oracle import binding as B
from tests import opq_ref as OR
from tests.parity import compare_exact

pytestmark = pytest.mark.gpu

D_, NLIST, M_, N_ = 32, 16, 8, 4000
PARAM = '{"ncentroids": %d, "nsubvector": %d, "opq": {"nsubvector": 8}, "nprobe": 6, "metric_type": "L2"}' % (NLIST, M_)
PLAIN = '{"ncentroids": %d, "nsubvector": %d, "nprobe": 6, "metric_type": "L2"}' % (NLIST, M_)
RP = '{"metric_type": "L2", "recall_num": 40, "nprobe": 6}'


def _model(param=PARAM, indexing_size=3000):
    from gamma_amd import plugin
    return plugin.PluginModel("HIPIVFPQ", D_, param, indexing_size=indexing_size)


def _index_file(root):
    for dp, _, files in os.walk(str(root)):
        if "ivfpq.index" in files:
            return os.path.join(dp, "ivfpq.index")
    raise AssertionError("no ivfpq.index under %s" % root)


def _searches(m, o, base, A, seed):
    out = []
    for nq in (1, 8, 25, 300):
        for has_rank in (True, False):
            q = OR.pick_queries(o, base, A, OR.clustered(nq + 20, D_, seed + nq), nq, 10, 6, 40, B.METRIC_L2)
            D, I, _ = OR.search_ref(o, base, q, OR.apply_chain(A, q), 10, 6, 40, has_rank, B.METRIC_L2)
            Dm, Im = m.search(q, 10, RP, has_rank=has_rank)
            compare_exact(D, I, Dm, Im)
            out.append((q, has_rank, Dm, Im))
    return out


def test_plugin_opq_indexing_add_update_search_dump_load(tmp_path):
    from gamma_amd import plugin
    base = OR.clustered(N_, D_, 5)
    m, m2 = _model(), _model()
    try:
        m.store(base)
        assert m.opq_matrix() is None
        assert m.indexing() == 0
        A = m.opq_matrix()
        assert A is not None and OR.orthonormality_defect(A) <= 4 * OR.U
        cc, pq = m.trained_state(NLIST, M_)
        # Indexing trains the quantizers on the ROTATED training set (the first indexing_size vectors)
        rot = OR.apply_chain(A, base)
        rc_, rp_ = B.ivfpq_train(rot[:3000], NLIST, M_)
        assert cc.tobytes() == rc_.tobytes() and pq.tobytes() == rp_.tobytes()
        o = B.OracleIVFPQ(D_, NLIST, M_, 8, B.METRIC_L2)
        o.set_trained(cc, pq, None)
        B.lib().go_set_assign_mode(-1)
        for i0 in range(0, N_, 1500):                  # engine-sized batches
            assert m.add(base[i0:i0 + 1500])
            assert o.add(rot[i0:i0 + 1500])
        _searches(m, o, base, A, 500)
        # Update: re-encoded from the rotated vector, re-ranked on the raw one
        base = base.copy()
        rng = np.random.default_rng(4)
        for vid in rng.choice(N_, 12, replace=False):
            vid = int(vid)
            newv = OR.clustered(1, D_, 9000 + vid)[0]
            assert m.update(vid, newv) == 0
            B.lib().go_set_assign_mode(0)
            o.update(vid, OR.apply_chain(A, newv[None, :]))
            B.lib().go_set_assign_mode(-1)
            base[vid] = newv
        res = _searches(m, o, base, A, 700)
        # Dump / Load into a fresh model: matrix, trained state and results are the same bytes
        assert m.dump(str(tmp_path)) == 0
        m2.store(base)
        assert m2.load(str(tmp_path)) == N_
        assert m2.opq_matrix().tobytes() == A.tobytes()
        cc2, pq2 = m2.trained_state(NLIST, M_)
        assert cc2.tobytes() == cc.tobytes() and pq2.tobytes() == pq.tobytes()
        for q, has_rank, Dm, Im in res:
            D2, I2 = m2.search(q, 10, RP, has_rank=has_rank)
            assert D2.tobytes() == Dm.tobytes() and np.array_equal(I2, Im)
        # the bytes between the product quantizer and the lists are the record of index/gamma_index_io.cc:225-240
        path = _index_file(tmp_path)
        data = open(path, "rb").read()
        hdr = 4 + 8 + 8 + 8 + 1 + 4                                       # index header: d, ntotal, 2 x i64, is_trained, metric
        off = 4 + hdr + 8 + 8 + 4 + hdr + 8 + 4 * NLIST * D_ + 1 + 8      # .. quantizer, direct map
        off += 1 + 8 + 8 + 8 + 8 + 8 + 4 * M_ * 256 * (D_ // M_)          # by_residual, code_size, pq (d, M, nbits, centroids)
        rec = (b"LTra" + b"\x00" + struct.pack("<Q", D_ * D_) + A.tobytes() + struct.pack("<Q", 0) + struct.pack("<ii", D_, D_)
               + b"\x01")
        assert data[off:off + len(rec)] == rec
        assert data[off + len(rec):off + len(rec) + 4] == b"ilar"
        # a file with the record on a model without "opq", and a file without it on a model with "opq": rejected
        plain = _model(PLAIN)
        try:
            plain.store(base)
            assert plain.load(str(tmp_path)) == -1
        finally:
            plain.close()
        assert plugin.iwpq_rewrite_opq(path, path, None) == 0
        assert plugin.iwpq_read_opq(path, D_) == (0, None)
        m3 = _model()
        try:
            m3.store(base)
            assert m3.load(str(tmp_path)) == -1
        finally:
            m3.close()
    finally:
        m.close()
        m2.close()


@pytest.mark.parametrize("param", [
    '{"ncentroids": 16, "nsubvector": 8, "opq": {"nsubvector": 8}, "devices": "0,0"}',
    '{"ncentroids": 16, "nsubvector": 8, "opq": {"nsubvector": 8}, "nbits_per_idx": 4}',
    '{"ncentroids": 16, "nsubvector": 8, "opq": {"nsubvector": 5}}'], ids=["devices", "4bit", "indivisible"])
def test_plugin_opq_init_rejects(param):
    with pytest.raises(_lib.GammaHipError, match="returned -2"):
        _model(param)
