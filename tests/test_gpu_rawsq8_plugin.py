"""GPU: the HIPIVFPQ plugin with "raw_dtype": "sq8", driven like VectorManager drives a model (Init, Indexing, Add, Search,
Update, Delete, Dump, Load).  Indexing() trains the store's ranges on the rows it trains the quantizers with; with W = the rows
those ranges store (tests/sq8_ref.py) the model must answer what the CPU oracle that lists the fp32 vectors and re-ranks over W
answers, labels and distance bits at every rank.  Only the store is quantised: without the re-rank (has_rank off) the model
answers byte for byte what the fp32 model with the same trained state answers, and its ivfpq.index is the fp32 model's."""
import os
import shutil
import struct

import numpy as np
import pytest

from gamma_amd import _lib
from oracle import binding as B
from tests import sq8_ref as S
from tests.parity import compare_exact

pytestmark = pytest.mark.gpu

D_, NLIST, M_, N_ = 32, 16, 8, 6000
NTRAIN = 3000
WIDE = dict(min_score=-3e38, max_score=3e38)
SQ8 = ', "raw_dtype": "sq8"'


def make_base(seed, n=N_):
    return np.concatenate([S.rows(n // 2, D_, seed), S.rows(n - n // 2, D_, seed + 1, wide=1.6)])


def _param(metric="L2", extra=""):
    return '{"ncentroids": %d, "nsubvector": %d, "nprobe": 8, "metric_type": "%s"%s}' % (NLIST, M_, metric, extra)


def _model(param, indexing_size=NTRAIN, name="HIPIVFPQ"):
    from gamma_amd import plugin
    return plugin.PluginModel(name, D_, param, indexing_size=indexing_size)


def _search(m, q, req, **kw):
    return m.search(q, 10, req, **WIDE, **kw)


def _indexed_pair(base, metric="L2", key=SQ8):
    """an sq8 model that ran Indexing() over the engine's first NTRAIN rows, its ranges (checked against numpy), the rows W they
    store, an fp32 model (nothing stored yet) and the sq8 model's trained state"""
    m, m32 = _model(_param(metric, key)), _model(_param(metric))
    m.store(base)
    assert m.sq8_ranges() is None
    assert m.indexing() == 0
    vmin, vmax = m.sq8_ranges()
    assert np.array_equal(vmin, base[:NTRAIN].min(axis=0)) and np.array_equal(vmax, base[:NTRAIN].max(axis=0))
    W = S.stored(base, vmin, vmax)
    cc, pq = m.trained_state(NLIST, M_)
    return m, m32, vmin, vmax, W, cc, pq


@pytest.mark.parametrize("metric,bm", [("L2", B.METRIC_L2), ("InnerProduct", B.METRIC_IP)], ids=["l2", "ip"])
def test_plugin_add_search_update_delete(metric, bm):
    base = make_base(3)
    q = S.rows(48, D_, 9)
    req = '{"metric_type": "%s", "recall_num": 100, "nprobe": 8}' % metric
    m, m32, vmin, vmax, W, cc, pq = _indexed_pair(base, metric, ', "raw_dtype": "SQ8"')
    try:
        m32.store(base)
        assert m32.set_trained(cc, pq) == 0
        o = B.OracleIVFPQ(D_, NLIST, M_, 8, bm)
        o.set_trained(cc, pq, None)
        assert m.add(base[:3000]) and m32.add(base[:3000])
        B.lib().go_set_assign_mode(1)          # GammaIVFPQIndex::Add of >= 20 vectors: faiss's BLAS assign rule
        try:
            assert o.add(base[:3000])
            # an Add with a row the store refuses fails, and lists nothing: the model answers as before, and the same vectors
            # are added afterwards at the same vids
            D0, I0 = _search(m, q, req)
            bad = base[3000:].copy()
            bad[1500, 7] = np.nan
            assert not m.add(bad)
            D1, I1 = _search(m, q, req)
            assert D1.tobytes() == D0.tobytes() and I1.tobytes() == I0.tobytes() and I1.max() < 3000
            assert m.add(base[3000:]) and m32.add(base[3000:])
            assert o.add(base[3000:])
        finally:
            B.lib().go_set_assign_mode(0)
        o.set_raw(W)
        ctx = B.make_ctx(**WIDE)

        def same_lists(qq):
            """without the re-rank nothing reads the store: the fp32 model's answer, byte for byte"""
            Dm, Im = _search(m, qq, req, has_rank=False)
            D32, I32 = _search(m32, qq, req, has_rank=False)
            assert Dm.tobytes() == D32.tobytes() and Im.tobytes() == I32.tobytes()
            return Dm, Im

        for n in (len(q), 7):              # GEMM-form coarse, exact coarse
            D, I = o.search(q[:n], 10, 8, recall_num=100, has_rank=True, metric=bm, ctx=ctx, coarse_mode=-1)
            compare_exact(D, I, *_search(m, q[:n], req))
            D, I = o.search(q[:n], 10, 8, recall_num=100, has_rank=False, metric=bm, ctx=ctx, coarse_mode=-1)
            compare_exact(D, I, *same_lists(q[:n]))
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
        Dm, Im = _search(m, q, req)
        compare_exact(D, I, Dm, Im)
        assert not np.isin(Im, dead).any()
        same_lists(q)
        # Update: re-encode, move between lists, the row rewritten; a row the store refuses fails the Update and changes nothing
        rng = np.random.default_rng(4)
        raw = W.copy()
        live = [int(v) for v in rng.choice(N_, 12, replace=False) if int(v) not in set(dead.tolist())]
        inf = S.rows(1, D_, 999)[0]
        inf[3] = np.inf
        assert m.update(live[0], inf) != 0
        Dm1, Im1 = _search(m, q, req)
        assert Dm1.tobytes() == Dm.tobytes() and Im1.tobytes() == Im.tobytes()
        same_lists(q)
        for vid in live:
            newv = S.rows(1, D_, 1000 + vid, wide=1.5)[0]
            assert m.update(vid, newv) == 0 and m32.update(vid, newv) == 0
            o.update(vid, newv)
            raw[vid] = S.stored(newv[None, :], vmin, vmax)[0]
        o.set_raw(raw)
        D, I = o.search(q, 10, 8, recall_num=100, has_rank=True, metric=bm, ctx=ctx, coarse_mode=-1)
        Dm, Im = _search(m, q, req)
        compare_exact(D, I, Dm, Im)
        same_lists(q)
        # brute force reads fp32 rows: refused, the model keeps serving
        with pytest.raises(_lib.GammaHipError):
            m.search(q[:4], 10, req, brute_force=True, **WIDE)
        Dm2, Im2 = _search(m, q, req)
        assert Dm2.tobytes() == Dm.tobytes() and np.array_equal(Im2, Im)
    finally:
        m.close()
        m32.close()


def test_plugin_indexing_dump_load(tmp_path):
    """Indexing trains the quantizers on the engine's fp32 vectors (the same trained state as the fp32 model's) and the ranges on
    the same rows; Dump writes ivfpq.index as the fp32 model does, byte for byte, and the ranges beside it; Load sets them before
    the mirror is re-encoded from the engine's store"""
    base = make_base(100 + D_)
    q = S.rows(30, D_, 10)
    req = '{"metric_type": "L2", "recall_num": 100, "nprobe": 8}'
    m, m32, vmin, vmax, W, cc, pq = _indexed_pair(base)
    m2, m3, m4 = _model(_param(extra=SQ8)), _model(_param(extra=SQ8)), _model(_param(extra=SQ8))
    try:
        m32.store(base)
        assert m32.indexing() == 0
        cc32, pq32 = m32.trained_state(NLIST, M_)
        assert cc.tobytes() == cc32.tobytes() and pq.tobytes() == pq32.tobytes()
        assert m.add(base) and m32.add(base)
        D1, I1 = _search(m, q, req)
        Dn, In = _search(m, q, req, has_rank=False)
        D32, I32 = _search(m32, q, req, has_rank=False)           # without the re-rank the store is not read
        assert Dn.tobytes() == D32.tobytes() and In.tobytes() == I32.tobytes()
        o = B.OracleIVFPQ(D_, NLIST, M_, 8, B.METRIC_L2)
        o.set_trained(cc, pq, None)
        B.lib().go_set_assign_mode(1)
        try:
            assert o.add(base)
        finally:
            B.lib().go_set_assign_mode(0)
        o.set_raw(W)
        D, I = o.search(q, 10, 8, recall_num=100, has_rank=True, metric=B.METRIC_L2, ctx=B.make_ctx(**WIDE), coarse_mode=-1)
        compare_exact(D, I, D1, I1)
        d8, d32 = tmp_path / "sq8", tmp_path / "f32"
        d8.mkdir()
        d32.mkdir()
        assert m.dump(str(d8)) == 0 and m32.dump(str(d32)) == 0
        idx8 = [os.path.join(r, f) for r, _, fs in os.walk(d8) for f in fs if f == "ivfpq.index"]
        idx32 = [os.path.join(r, f) for r, _, fs in os.walk(d32) for f in fs if f == "ivfpq.index"]
        assert len(idx8) == 1 and len(idx32) == 1
        assert open(idx8[0], "rb").read() == open(idx32[0], "rb").read()
        side = os.path.join(os.path.dirname(idx8[0]), "raw_sq8.ranges")
        blob = open(side, "rb").read()
        assert len(blob) == 8 + 8 * D_ and struct.unpack("<i", blob[4:8])[0] == D_
        assert blob[8:8 + 4 * D_] == vmin.tobytes() and blob[8 + 4 * D_:] == vmax.tobytes()
        assert not os.path.exists(os.path.join(os.path.dirname(idx32[0]), "raw_sq8.ranges"))
        # Load into a fresh model: the same ranges, the same answers
        m2.store(base)
        assert m2.load(str(d8)) == len(base)
        a, b = m2.sq8_ranges()
        assert a.tobytes() == vmin.tobytes() and b.tobytes() == vmax.tobytes()
        D2, I2 = _search(m2, q, req)
        assert D1.tobytes() == D2.tobytes() and np.array_equal(I1, I2)
        # without the side file, and with the ranges of another d: refused
        gone = tmp_path / "gone"
        shutil.copytree(d8, gone)
        os.remove(side.replace(str(d8), str(gone)))
        m3.store(base)
        assert m3.load(str(gone)) < 0
        other = tmp_path / "other"
        shutil.copytree(d8, other)
        with open(side.replace(str(d8), str(other)), "wb") as f:
            f.write(blob[:4] + struct.pack("<i", D_ + 1) + blob[8:] + b"\0" * 8)
        m4.store(base)
        assert m4.load(str(other)) < 0
        magic = tmp_path / "magic"
        shutil.copytree(d8, magic)
        with open(side.replace(str(d8), str(magic)), "wb") as f:
            f.write(b"XXXX" + blob[4:])
        assert m4.load(str(magic)) < 0
    finally:
        for mm in (m, m2, m3, m4, m32):
            mm.close()


def test_plugin_memory_accounting(monkeypatch):
    """GetTotalMemBytes reports rows of 1 byte per element plus the store's tables (16 bytes per dimension).  Capacity rounding:
    under GAMMA_HIP_NO_RAW_VMM the store's capacity is max(rows needed, 1.5 x its capacity, 1024) ROWS, the same number for both
    models, so the two models differ by capacity x d x 3 bytes less the tables, with n <= capacity <= 1.5 n."""
    monkeypatch.setenv("GAMMA_HIP_NO_RAW_VMM", "1")
    base = make_base(5)
    mem = {}
    cc = pq = None
    for name, extra in (("sq8", SQ8), ("f32", ', "raw_dtype": "float32"')):
        m = _model(_param(extra=extra))
        try:
            m.store(base)
            if cc is None:
                assert m.indexing() == 0
                cc, pq = m.trained_state(NLIST, M_)
            else:
                assert m.set_trained(cc, pq) == 0
            for i0 in range(0, N_, 3000):
                assert m.add(base[i0:i0 + 3000])
            mem[name] = m.mem_bytes()
        finally:
            m.close()
    diff = mem["f32"] - mem["sq8"] + 16 * D_
    assert diff % (D_ * 3) == 0 and N_ * D_ * 3 <= diff <= N_ * D_ * 3 * 3 // 2, (mem, diff)


def test_plugin_untrained_model_refuses_to_search():
    """before training the model answers by brute force over the mirror, which reads fp32 rows: with sq8 rows that is an error,
    as a brute_force_search request is"""
    base = make_base(6, n=500)
    m = _model(_param(extra=SQ8))
    try:
        m.store(base)
        with pytest.raises(_lib.GammaHipError):
            m.search(base[:4], 5, '{"metric_type": "L2"}', **WIDE)
    finally:
        m.close()


def test_plugin_key_rejections():
    with pytest.raises(_lib.GammaHipError):
        _model(_param(extra=SQ8 + ', "devices": "0,0"'))
    for bad in ("sq4", "sq", "scalar8"):
        with pytest.raises(_lib.GammaHipError):
            _model(_param(extra=', "raw_dtype": "%s"' % bad))
    m = _model(_param(extra=', "raw_dtype": "Sq8"'))
    m.close()
    # HIPFLAT and HIPIVFFLAT keep rejecting the value
    with pytest.raises(_lib.GammaHipError):
        _model('{"metric_type": "L2", "raw_dtype": "sq8"}', name="HIPFLAT")
    with pytest.raises(_lib.GammaHipError):
        _model('{"ncentroids": %d, "nprobe": 8, "metric_type": "L2", "raw_dtype": "sq8"}' % NLIST, name="HIPIVFFLAT")
