"""GPU: the HIPIVFPQ plugin with "raw_dtype": "float16", driven like VectorManager drives a model (Init, Add, Search, Update,
Delete, Indexing, Dump, Load) against the CPU oracle that adds the fp32 vectors and re-ranks on the ROUNDED rows."""
import numpy as np
import pytest

from gamma_amd import _lib
from oracle import binding as B
from tests.parity import compare_exact

pytestmark = pytest.mark.gpu

D_, NLIST, M_, N_ = 32, 16, 8, 6000
WIDE = dict(min_score=-3e38, max_score=3e38)


def rounded(x):
    return np.ascontiguousarray(x, dtype=np.float32).astype(np.float16).astype(np.float32)


def gauss3(n, d, seed):
    return (3.0 * np.random.default_rng(seed).standard_normal((n, d))).astype(np.float32)


def _param(metric="L2", extra=', "raw_dtype": "float16"'):
    return '{"ncentroids": %d, "nsubvector": %d, "nprobe": 8, "metric_type": "%s"%s}' % (NLIST, M_, metric, extra)


def _model(param, indexing_size=3000):
    from gamma_amd import plugin
    return plugin.PluginModel("HIPIVFPQ", D_, param, indexing_size=indexing_size)


@pytest.mark.parametrize("metric,bm", [("L2", B.METRIC_L2), ("InnerProduct", B.METRIC_IP)], ids=["l2", "ip"])
def test_plugin_add_search_update_delete_equal_the_oracle_on_rounded_rows(metric, bm):
    base = gauss3(N_, D_, 3)
    q = gauss3(48, D_, 9)
    cc, pq = B.ivfpq_train(base[:3000], NLIST, M_)
    req = '{"metric_type": "%s", "recall_num": 100, "nprobe": 8}' % metric
    m = _model(_param(metric))
    try:
        m.store(base)
        assert m.set_trained(cc, pq) == 0
        o = B.OracleIVFPQ(D_, NLIST, M_, 8, bm)
        o.set_trained(cc, pq, None)
        B.lib().go_set_assign_mode(1)          # GammaIVFPQIndex::Add of >= 20 vectors: faiss's BLAS assign rule
        try:
            for i0 in range(0, N_, 3000):      # two batches
                assert m.add(base[i0:i0 + 3000])
                assert o.add(base[i0:i0 + 3000])
        finally:
            B.lib().go_set_assign_mode(0)
        raw = rounded(base)
        o.set_raw(raw)
        ctx = B.make_ctx(**WIDE)
        D32 = None
        for has_rank in (True, False):
            for n in (len(q), 7):              # GEMM-form coarse, exact coarse
                D, I = o.search(q[:n], 10, 8, recall_num=100, has_rank=has_rank, metric=bm, ctx=ctx, coarse_mode=-1)
                Dm, Im = m.search(q[:n], 10, req, has_rank=has_rank, **WIDE)
                compare_exact(D, I, Dm, Im)
        # the rounded rows are what is compared: the fp32-row oracle says something else
        o.set_raw(base)
        D32, _ = o.search(q, 10, 8, recall_num=100, has_rank=True, metric=bm, ctx=ctx, coarse_mode=-1)
        o.set_raw(raw)
        D, I = o.search(q, 10, 8, recall_num=100, has_rank=True, metric=bm, ctx=ctx, coarse_mode=-1)
        assert D.tobytes() != D32.tobytes()
        # Delete
        dead = np.unique(I[:, 0])
        dead = dead[dead >= 0]
        assert m.delete(dead) == 0
        bmap = np.zeros(N_ // 8 + 1, np.uint8)
        np.bitwise_or.at(bmap, dead >> 3, (1 << (dead & 7)).astype(np.uint8))
        o.delete(dead)
        ctx = B.make_ctx(docids_bitmap=bmap, **WIDE)
        D, I = o.search(q, 10, 8, recall_num=100, has_rank=True, metric=bm, ctx=ctx, coarse_mode=-1)
        Dm, Im = m.search(q, 10, req, **WIDE)
        compare_exact(D, I, Dm, Im)
        assert not np.isin(Im, dead).any()
        # Update: re-encode, move between lists, the row rewritten (rounded)
        rng = np.random.default_rng(4)
        raw = raw.copy()
        for vid in rng.choice(N_, 12, replace=False):
            vid = int(vid)
            if vid in set(dead.tolist()):
                continue
            newv = gauss3(1, D_, 1000 + vid)[0]
            assert m.update(vid, newv) == 0
            o.update(vid, newv)
            raw[vid] = rounded(newv)
        o.set_raw(raw)
        D, I = o.search(q, 10, 8, recall_num=100, has_rank=True, metric=bm, ctx=ctx, coarse_mode=-1)
        Dm, Im = m.search(q, 10, req, **WIDE)
        compare_exact(D, I, Dm, Im)
        # brute force reads fp32 rows: refused, the model keeps serving
        with pytest.raises(_lib.GammaHipError):
            m.search(q[:4], 10, req, brute_force=True, **WIDE)
        Dm2, Im2 = m.search(q, 10, req, **WIDE)
        assert Dm2.tobytes() == Dm.tobytes() and np.array_equal(Im2, Im)
    finally:
        m.close()


@pytest.mark.parametrize("metric,bm", [("L2", B.METRIC_L2), ("InnerProduct", B.METRIC_IP)], ids=["l2", "ip"])
def test_plugin_indexing_dump_load(tmp_path, metric, bm):
    """Indexing trains on the engine's fp32 vectors (the same trained state as the fp32 model's); Dump / Load are unchanged:
    the mirror comes back from the engine's store and is rounded on upload"""
    base = gauss3(N_, D_, 100 + D_)
    q = gauss3(30, D_, 10)
    req = '{"metric_type": "%s", "recall_num": 100, "nprobe": 8}' % metric
    m, m2, m32 = _model(_param(metric), 5000), _model(_param(metric), 5000), _model(_param(metric, extra=""), 5000)
    try:
        m.store(base)
        m32.store(base)
        assert m.indexing() == 0 and m32.indexing() == 0
        cc, pq = m.trained_state(NLIST, M_)
        cc32, pq32 = m32.trained_state(NLIST, M_)
        assert cc.tobytes() == cc32.tobytes() and pq.tobytes() == pq32.tobytes()
        assert m.add(base) and m32.add(base)
        D1, I1 = m.search(q, 10, req, **WIDE)
        # without rank nothing of the raw store is read: the two models agree; with rank they do not (rounded rows)
        Dn, In = m.search(q, 10, req, has_rank=False, **WIDE)
        Dn32, In32 = m32.search(q, 10, req, has_rank=False, **WIDE)
        assert Dn.tobytes() == Dn32.tobytes() and np.array_equal(In, In32)
        assert D1.tobytes() != m32.search(q, 10, req, **WIDE)[0].tobytes()
        # the oracle over the model's own trained state and the rounded rows
        o = B.OracleIVFPQ(D_, NLIST, M_, 8, bm)
        o.set_trained(cc, pq, None)
        B.lib().go_set_assign_mode(1)
        try:
            assert o.add(base)
        finally:
            B.lib().go_set_assign_mode(0)
        o.set_raw(rounded(base))
        D, I = o.search(q, 10, 8, recall_num=100, has_rank=True, metric=bm, ctx=B.make_ctx(**WIDE), coarse_mode=-1)
        compare_exact(D, I, D1, I1)
        assert m.dump(str(tmp_path)) == 0
        m2.store(base)
        assert m2.load(str(tmp_path)) == len(base)
        D2, I2 = m2.search(q, 10, req, **WIDE)
        assert D1.tobytes() == D2.tobytes() and np.array_equal(I1, I2)
    finally:
        m.close()
        m2.close()
        m32.close()


def test_plugin_memory_accounting(monkeypatch):
    """GetTotalMemBytes reports rows of 2 bytes per element.  Capacity rounding: under GAMMA_HIP_NO_RAW_VMM the store's
    capacity is max(rows needed, 1.5 x its capacity, 1024) ROWS, the same number for both models (the mapped store rounds
    to chunks of 64 MB instead, far more than these rows), so the two models differ by capacity x d x 2 bytes with
    n <= capacity <= 1.5 n."""
    monkeypatch.setenv("GAMMA_HIP_NO_RAW_VMM", "1")
    base = gauss3(N_, D_, 5)
    cc, pq = B.ivfpq_train(base[:3000], NLIST, M_)
    mem = {}
    for name, extra in (("f16", ', "raw_dtype": "float16"'), ("f32", ', "raw_dtype": "float32"')):
        m = _model(_param(extra=extra))
        try:
            m.store(base)
            assert m.set_trained(cc, pq) == 0
            for i0 in range(0, N_, 3000):
                assert m.add(base[i0:i0 + 3000])
            mem[name] = m.mem_bytes()
        finally:
            m.close()
    diff = mem["f32"] - mem["f16"]
    assert diff % (D_ * 2) == 0 and N_ * D_ * 2 <= diff <= N_ * D_ * 3, (mem, diff)


def test_plugin_untrained_model_refuses_to_search():
    """before training the model answers by brute force over the mirror, which reads fp32 rows: with float16 rows that is an
    error, as a brute_force_search request is; the fp32 model serves it"""
    base = gauss3(500, D_, 6)
    for extra, served in ((', "raw_dtype": "float16"', False), ("", True)):
        m = _model(_param(extra=extra))
        try:
            m.store(base)
            if served:
                m.search(base[:4], 5, '{"metric_type": "L2"}', **WIDE)
            else:
                with pytest.raises(_lib.GammaHipError):
                    m.search(base[:4], 5, '{"metric_type": "L2"}', **WIDE)
        finally:
            m.close()


def test_plugin_key_rejections():
    with pytest.raises(_lib.GammaHipError):
        _model(_param(extra=', "raw_dtype": "bfloat16"'))
    with pytest.raises(_lib.GammaHipError):
        _model(_param(extra=', "raw_dtype": "float16", "devices": "0,0"'))
    m = _model(_param(extra=', "raw_dtype": "float32"'))   # the default, spelled out
    m.close()
