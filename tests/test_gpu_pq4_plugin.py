"""GPU: the HIPIVFPQ plugin with "nbits_per_idx": 4, driven like VectorManager drives a model (Init, Indexing, Add, Search,
Update, Delete, Dump, Load) against the yardstick of tests/pq4_ref.py and the C ABI path, and its Dump against the bytes
faiss::write_index produced for such an index (tests/golden/ivfpq4_iwpq_small.npz)."""
import os

import numpy as np
import pytest

from gamma_amd import api
from tests import gen_golden_pq4 as GG
from tests import pq4_ref as PR
from tests.parity import compare_exact

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
D_, NLIST, M_, N_ = 32, 16, 8, 4000
PARAM = '{"ncentroids": %d, "nsubvector": %d, "nbits_per_idx": 4, "nprobe": 6, "metric_type": "L2"}' % (NLIST, M_)


def _model(indexing_size=3000, d=D_, param=PARAM):
    from gamma_amd import plugin
    return plugin.PluginModel("HIPIVFPQ", d, param, indexing_size=indexing_size)


def test_plugin_4bit_add_search_update_delete_equal_the_yardstick_and_the_abi():
    base = PR.clustered(N_, D_, 3)
    q = PR.clustered(48, D_, 9)
    cc, pq = PR.train(base[:3000], NLIST, M_)
    m = _model()
    g = api.GammaHip(0)
    try:
        m.store(base)
        assert m.set_trained(cc, pq) == 0
        lists = None
        for i0 in range(0, N_, 1500):     # engine-sized batches: each assigned by the form its own size selects
            assert m.add(base[i0:i0 + 1500])
            lno, codes = PR.encode(base[i0:i0 + 1500], cc, pq)
            lists = PR.build_lists(lno, codes, NLIST, first_vid=i0, lists=lists)
        ix = PR.Index(cc, pq, lists, raw=base.copy())
        g.ivfpq4_init(D_, NLIST, M_, api.METRIC_L2)
        g.ivfpq_set_trained(cc, pq, None)
        g.raw_init(D_)
        g.raw_append(base)
        for i0 in range(0, N_, 1500):
            g.add(base[i0:i0 + 1500], i0)
        for has_rank in (True, False):
            for n in (len(q), 7):
                D, I, _ = ix.search(q[:n], 10, 6, recall_num=100, has_rank=has_rank)
                Dm, Im = m.search(q[:n], 10, '{"metric_type": "L2", "recall_num": 100, "nprobe": 6}', has_rank=has_rank)
                compare_exact(D, I, Dm, Im)
                Dg, Ig = g.ivfpq_search(q[:n], 10, api.SearchArgs(metric=api.METRIC_L2, nprobe=6, recall_num=100,
                                                                  has_rank=has_rank))
                assert Dm.tobytes() == Dg.tobytes() and np.array_equal(Im, Ig), "plugin vs the ABI path"
        # Delete
        D, I, _ = ix.search(q, 10, 6, recall_num=100)
        dead = np.unique(I[:, 0])
        dead = dead[dead >= 0]
        assert m.delete(dead) == 0
        filt = PR.Filter(deleted=dead)
        D, I, _ = ix.search(q, 10, 6, recall_num=100, filt=filt)
        Dm, Im = m.search(q, 10, "")
        compare_exact(D, I, Dm, Im)
        assert not np.isin(Im, dead).any()
        # Update: re-encode, move between lists
        rng = np.random.default_rng(4)
        for vid in rng.choice(N_, 12, replace=False):
            vid = int(vid)
            if vid in set(dead.tolist()):
                continue
            newv = base[(vid + 17) % N_].copy()
            assert m.update(vid, newv) == 0
            ix.update(vid, newv)
            ix.raw[vid] = newv
        D, I, _ = ix.search(q, 10, 6, recall_num=100, filt=filt)
        Dm, Im = m.search(q, 10, "")
        compare_exact(D, I, Dm, Im)
    finally:
        m.close()
        g.close()


def test_plugin_4bit_indexing_trains_16_centroids(tmp_path):
    base = PR.clustered(5000, D_, 100 + D_)
    q = PR.clustered(30, D_, 10)
    m = _model(indexing_size=5000)
    m2 = _model(indexing_size=5000)
    try:
        m.store(base)
        assert m.indexing() == 0
        cc, pq = m.trained_state(NLIST, M_, ksub=16)
        # the training set is the first min(indexing_size, 256 * nlist) vectors (gamma_index_ivfpq.cc:280-301): 4096 here
        rc, rp = PR.train(base[:256 * NLIST], NLIST, M_)
        assert cc.tobytes() == rc.tobytes() and pq.tobytes() == rp.tobytes()
        assert m.add(base)
        D1, I1 = m.search(q, 10, '{"metric_type": "L2", "recall_num": 100, "nprobe": 8}')
        # Dump / Load round trip
        assert m.dump(str(tmp_path)) == 0
        m2.store(base)
        assert m2.load(str(tmp_path)) == len(base)
        cc2, pq2 = m2.trained_state(NLIST, M_, ksub=16)
        assert cc.tobytes() == cc2.tobytes() and pq.tobytes() == pq2.tobytes()
        D2, I2 = m2.search(q, 10, '{"metric_type": "L2", "recall_num": 100, "nprobe": 8}')
        assert D1.tobytes() == D2.tobytes() and np.array_equal(I1, I2)
        # a file whose nbits / code_size disagree with the model is rejected: the 8-bit model cannot load it
        from gamma_amd import plugin
        m8 = plugin.PluginModel("HIPIVFPQ", D_, '{"ncentroids": %d, "nsubvector": %d, "nprobe": 6, "metric_type": "L2"}'
                                % (NLIST, M_), indexing_size=5000)
        try:
            m8.store(base)
            assert m8.load(str(tmp_path)) < 0
        finally:
            m8.close()
    finally:
        m.close()
        m2.close()


def test_plugin_4bit_dump_is_what_faiss_writes_and_loads_it(tmp_path):
    z = np.load(os.path.join(HERE, "golden", "ivfpq4_iwpq_small.npz"))
    d, nlist, M, N = int(z["d"]), int(z["nlist"]), int(z["M"]), int(z["N"])
    base = z["base"]
    param = '{"ncentroids": %d, "nsubvector": %d, "nbits_per_idx": 4, "nprobe": 5, "metric_type": "L2"}' % (nlist, M)
    want = z["file_bytes"].copy()
    want[8:16] = 0   # faiss's ntotal; GammaIVFPQIndex never advances it and its dumps carry 0 (as the 8-bit Dump does)
    # Add (the plugin's own encode), then Dump: the file faiss::write_index wrote for the same index
    m = _model(indexing_size=N, d=d, param=param)
    try:
        m.store(base)
        assert m.set_trained(z["cc"], z["pq"]) == 0
        assert m.add(base)
        out = tmp_path / "dump"
        os.makedirs(out)
        assert m.dump(str(out)) == 0
        got = np.frombuffer(open(out / "vec.000" / "ivfpq.index", "rb").read(), dtype=np.uint8)
        assert got.size == want.size and got.tobytes() == want.tobytes()
    finally:
        m.close()
    # Load of faiss's own bytes, then a search against the yardstick on the same lists
    src = tmp_path / "src"
    os.makedirs(src / "vec.000")
    open(src / "vec.000" / "ivfpq.index", "wb").write(z["file_bytes"].tobytes())
    m = _model(indexing_size=N, d=d, param=param)
    try:
        m.store(base)
        assert m.load(str(src)) == N
        ix = PR.Index(z["cc"], z["pq"], GG.lists_of(z), raw=base)
        q = PR.clustered(40, d, 77)
        for has_rank in (True, False):
            D, I, _ = ix.search(q, 10, 5, recall_num=50, has_rank=has_rank)
            Dm, Im = m.search(q, 10, '{"metric_type": "L2", "recall_num": 50}', has_rank=has_rank)
            compare_exact(D, I, Dm, Im)
    finally:
        m.close()


def test_plugin_4bit_rejected_with_devices_and_other_nbits():
    from gamma_amd import _lib, plugin
    with pytest.raises(_lib.GammaHipError):
        plugin.PluginModel("HIPIVFPQ", D_, PARAM[:-1] + ', "devices": "0,0"}')
    with pytest.raises(_lib.GammaHipError):
        plugin.PluginModel("HIPIVFPQ", D_, '{"ncentroids": 16, "nsubvector": 8, "nbits_per_idx": 6}')
