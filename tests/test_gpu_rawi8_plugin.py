"""GPU: the HIPIVFPQ plugin with "raw_dtype": "uint8" | "int8", driven like VectorManager drives a model (Init, Add, Search,
Update, Delete, Indexing, Dump, Load).  The byte store is lossless, so the model must answer byte for byte what the fp32 model
answers, and what the CPU oracle over the untouched fp32 vectors answers."""
import numpy as np
import pytest

from gamma_amd import _lib
from oracle import binding as B
from tests.parity import compare_exact

pytestmark = pytest.mark.gpu

D_, NLIST, M_, N_ = 32, 16, 8, 6000
WIDE = dict(min_score=-3e38, max_score=3e38)
RANGE = {"uint8": (0, 255), "int8": (-128, 127)}
DTYPES = ["uint8", "int8"]


def ints(n, d, dtype, seed):
    lo, hi = RANGE[dtype]
    x = np.random.default_rng(seed).integers(lo, hi + 1, size=(n, d)).astype(np.float32)
    x[0, 0], x[0, -1] = lo, hi
    return x


def gauss(n, d, dtype, seed):
    lo, hi = RANGE[dtype]
    return ((lo + hi) / 2.0 + 60.0 * np.random.default_rng(seed).standard_normal((n, d))).astype(np.float32)


def _param(metric="L2", extra=""):
    return '{"ncentroids": %d, "nsubvector": %d, "nprobe": 8, "metric_type": "%s"%s}' % (NLIST, M_, metric, extra)


def _key(dtype):
    return ', "raw_dtype": "%s"' % dtype


def _model(param, indexing_size=3000):
    from gamma_amd import plugin
    return plugin.PluginModel("HIPIVFPQ", D_, param, indexing_size=indexing_size)


def _same(m, m32, q, req, **kw):
    Dm, Im = m.search(q, 10, req, **WIDE, **kw)
    D32, I32 = m32.search(q, 10, req, **WIDE, **kw)
    assert Dm.tobytes() == D32.tobytes() and Im.tobytes() == I32.tobytes()
    return Dm, Im


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("metric,bm", [("L2", B.METRIC_L2), ("InnerProduct", B.METRIC_IP)], ids=["l2", "ip"])
def test_plugin_add_search_update_delete_equal_the_fp32_model(metric, bm, dtype):
    base = ints(N_, D_, dtype, 3)
    q = gauss(48, D_, dtype, 9)
    cc, pq = B.ivfpq_train(base[:3000], NLIST, M_)
    req = '{"metric_type": "%s", "recall_num": 100, "nprobe": 8}' % metric
    m, m32 = _model(_param(metric, _key(dtype.upper() if dtype == "int8" else "UInt8"))), _model(_param(metric))
    try:
        o = B.OracleIVFPQ(D_, NLIST, M_, 8, bm)
        o.set_trained(cc, pq, None)
        for mm in (m, m32):
            mm.store(base)
            assert mm.set_trained(cc, pq) == 0
            assert mm.add(base[:3000])
        B.lib().go_set_assign_mode(1)          # GammaIVFPQIndex::Add of >= 20 vectors: faiss's BLAS assign rule
        try:
            assert o.add(base[:3000])
            # an Add with a row the store refuses fails, and lists nothing: the model answers as before, and the same vectors
            # are added afterwards at the same vids
            D0, I0 = _same(m, m32, q, req)
            bad = base[3000:].copy()
            bad[1500, 7] = 0.5
            assert not m.add(bad)
            D1, I1 = _same(m, m32, q, req)
            assert D1.tobytes() == D0.tobytes() and I1.tobytes() == I0.tobytes() and I1.max() < 3000
            assert m.add(base[3000:]) and m32.add(base[3000:])
            assert o.add(base[3000:])
        finally:
            B.lib().go_set_assign_mode(0)
        o.set_raw(base)
        ctx = B.make_ctx(**WIDE)
        for has_rank in (True, False):
            for n in (len(q), 7):              # GEMM-form coarse, exact coarse
                D, I = o.search(q[:n], 10, 8, recall_num=100, has_rank=has_rank, metric=bm, ctx=ctx, coarse_mode=-1)
                Dm, Im = _same(m, m32, q[:n], req, has_rank=has_rank)
                compare_exact(D, I, Dm, Im)
        # Delete
        D, I = o.search(q, 10, 8, recall_num=100, has_rank=True, metric=bm, ctx=ctx, coarse_mode=-1)
        dead = np.unique(I[:, 0])
        dead = dead[dead >= 0]
        assert m.delete(dead) == 0 and m32.delete(dead) == 0
        bmap = np.zeros(N_ // 8 + 1, np.uint8)
        np.bitwise_or.at(bmap, dead >> 3, (1 << (dead & 7)).astype(np.uint8))
        o.delete(dead)
        ctx = B.make_ctx(docids_bitmap=bmap, **WIDE)
        D, I = o.search(q, 10, 8, recall_num=100, has_rank=True, metric=bm, ctx=ctx, coarse_mode=-1)
        Dm, Im = _same(m, m32, q, req)
        compare_exact(D, I, Dm, Im)
        assert not np.isin(Im, dead).any()
        # Update: re-encode, move between lists, the row rewritten; a row the store refuses fails the Update and changes nothing
        rng = np.random.default_rng(4)
        raw = base.copy()
        live = [int(v) for v in rng.choice(N_, 12, replace=False) if int(v) not in set(dead.tolist())]
        frac = ints(1, D_, dtype, 999)[0]
        frac[3] += 0.25
        assert m.update(live[0], frac) != 0
        _same(m, m32, q, req)
        for vid in live:
            newv = ints(1, D_, dtype, 1000 + vid)[0]
            assert m.update(vid, newv) == 0 and m32.update(vid, newv) == 0
            o.update(vid, newv)
            raw[vid] = newv
        o.set_raw(raw)
        D, I = o.search(q, 10, 8, recall_num=100, has_rank=True, metric=bm, ctx=ctx, coarse_mode=-1)
        Dm, Im = _same(m, m32, q, req)
        compare_exact(D, I, Dm, Im)
        # brute force reads fp32 rows: refused, the model keeps serving
        with pytest.raises(_lib.GammaHipError):
            m.search(q[:4], 10, req, brute_force=True, **WIDE)
        Dm2, Im2 = m.search(q, 10, req, **WIDE)
        assert Dm2.tobytes() == Dm.tobytes() and np.array_equal(Im2, Im)
    finally:
        m.close()
        m32.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_plugin_indexing_dump_load(tmp_path, dtype):
    """Indexing trains on the engine's fp32 vectors (the same trained state as the fp32 model's); Dump / Load are unchanged:
    the mirror comes back from the engine's store and is converted on upload"""
    base = ints(N_, D_, dtype, 100 + D_)
    q = gauss(30, D_, dtype, 10)
    req = '{"metric_type": "L2", "recall_num": 100, "nprobe": 8}'
    m, m2, m32 = _model(_param(extra=_key(dtype)), 5000), _model(_param(extra=_key(dtype)), 5000), _model(_param(), 5000)
    try:
        m.store(base)
        m32.store(base)
        assert m.indexing() == 0 and m32.indexing() == 0
        cc, pq = m.trained_state(NLIST, M_)
        cc32, pq32 = m32.trained_state(NLIST, M_)
        assert cc.tobytes() == cc32.tobytes() and pq.tobytes() == pq32.tobytes()
        assert m.add(base) and m32.add(base)
        D1, I1 = _same(m, m32, q, req)
        _same(m, m32, q, req, has_rank=False)
        assert m.dump(str(tmp_path)) == 0
        m2.store(base)
        assert m2.load(str(tmp_path)) == len(base)
        D2, I2 = m2.search(q, 10, req, **WIDE)
        assert D1.tobytes() == D2.tobytes() and np.array_equal(I1, I2)
    finally:
        m.close()
        m2.close()
        m32.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_plugin_memory_accounting(monkeypatch, dtype):
    """GetTotalMemBytes reports rows of 1 byte per element.  Capacity rounding: under GAMMA_HIP_NO_RAW_VMM the store's
    capacity is max(rows needed, 1.5 x its capacity, 1024) ROWS, the same number for both models (the mapped store rounds
    to chunks of 64 MB instead, far more than these rows), so the two models differ by capacity x d x 3 bytes with
    n <= capacity <= 1.5 n."""
    monkeypatch.setenv("GAMMA_HIP_NO_RAW_VMM", "1")
    base = ints(N_, D_, dtype, 5)
    cc, pq = B.ivfpq_train(base[:3000], NLIST, M_)
    mem = {}
    for name, extra in (("i8", _key(dtype)), ("f32", ', "raw_dtype": "float32"')):
        m = _model(_param(extra=extra))
        try:
            m.store(base)
            assert m.set_trained(cc, pq) == 0
            for i0 in range(0, N_, 3000):
                assert m.add(base[i0:i0 + 3000])
            mem[name] = m.mem_bytes()
        finally:
            m.close()
    diff = mem["f32"] - mem["i8"]
    assert diff % (D_ * 3) == 0 and N_ * D_ * 3 <= diff <= N_ * D_ * 3 * 3 // 2, (mem, diff)


@pytest.mark.parametrize("dtype", DTYPES)
def test_plugin_untrained_model_refuses_to_search(dtype):
    """before training the model answers by brute force over the mirror, which reads fp32 rows: with byte rows that is an
    error, as a brute_force_search request is"""
    base = ints(500, D_, dtype, 6)
    m = _model(_param(extra=_key(dtype)))
    try:
        m.store(base)
        with pytest.raises(_lib.GammaHipError):
            m.search(base[:4], 5, '{"metric_type": "L2"}', **WIDE)
    finally:
        m.close()


def test_plugin_key_rejections():
    for dtype in DTYPES:
        with pytest.raises(_lib.GammaHipError):
            _model(_param(extra=_key(dtype) + ', "devices": "0,0"'))
    with pytest.raises(_lib.GammaHipError):
        _model(_param(extra=', "raw_dtype": "uint4"'))
    m = _model(_param(extra=', "raw_dtype": "Int8"'))
    m.close()
