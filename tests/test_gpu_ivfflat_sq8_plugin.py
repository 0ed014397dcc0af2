"""GPU: the HIPIVFFLAT plugin with "raw_dtype": "sq8", "sq8_ranges": "trained", driven like VectorManager drives a model (Init,
Indexing, Add, Search, Update, Delete, Dump, Load).  Indexing() trains the store's per-dimension ranges on the rows it trains the
coarse quantizer with; with W = the rows those ranges store (tests/sq8_ref.py) the model must answer
  * what the CPU oracle's IVFFLAT search answers over the lists of the caller's fp32 vectors with set_raw(W), labels and distance
    bits at every rank -- only the store is quantised, coarse assignment sees the caller's rows -- and
  * byte for byte what the fp32 HIPIVFFLAT model answers that holds W behind the same lists: the fp32 model LOADS the sq8 model's
    dump (ivfflat.index is the fp32 model's file: lists and vids) over an engine store that holds W."""
import os
import shutil
import struct

import numpy as np
import pytest

from gamma_amd import _lib
from oracle import binding as B
from tests import ivfflat_sq8_data as Q
from tests import sq8_ref as S
from tests.parity import compare_exact

pytestmark = pytest.mark.gpu

D_, N_, NLIST, P_ = 32, 3001, 16, 4
NTRAIN = N_ // 2      # Indexing() trains on the engine's first indexing_size rows: the half whose ranges ivfflat_sq8_data takes
METRIC = {"L2": B.METRIC_L2, "InnerProduct": B.METRIC_IP}
SQ8 = ', "raw_dtype": "sq8", "sq8_ranges": "trained"'


def data(seed):
    base, vmin, vmax = Q.base_rows(N_, D_, seed)
    W = np.ascontiguousarray(S.stored(base, vmin, vmax))
    return base, vmin, vmax, W, Q.queries(40, D_, seed + 2, W)      # 40 x 4 pairs: list-major; q[:5]: the small path


def _model(metric="L2", extra=""):
    from gamma_amd import plugin
    return plugin.PluginModel("HIPIVFFLAT", D_, '{"ncentroids": %d, "nprobe": %d, "metric_type": "%s"%s}'
                              % (NLIST, P_, metric, extra), indexing_size=NTRAIN)


def _indexed(base, vmin, vmax, metric="L2", extra=SQ8):
    """an sq8 model that ran Indexing() over the engine's first NTRAIN rows (its ranges checked against numpy) and its centroids"""
    m = _model(metric, extra)
    m.store(base)
    assert m.sq8_ranges() is None
    assert m.indexing() == 0
    a, b = m.sq8_ranges()
    assert np.array_equal(a, vmin) and np.array_equal(b, vmax)
    cc, _ = m.trained_state(NLIST, 1)
    return m, cc


def _oracle(cc, metric):
    o = B.OracleIVFPQ(D_, NLIST, 1, 8, METRIC[metric])
    o.set_trained(cc, np.zeros((256, D_), np.float32), None)
    return o


def _oracle_add(o, xb, i0):
    lno = B.ivfflat_assign(o, xb)
    order = np.argsort(lno, kind="stable")
    for l in np.unique(lno):
        sel = order[lno[order] == l]
        o.add_keys(int(l), i0 + sel, np.zeros((len(sel), 1), np.uint8))


def _fp32_twin(m, W, where, metric="L2"):
    """the fp32 model that holds W behind the sq8 model's lists: it loads the sq8 model's dump over an engine store of W"""
    assert m.dump(str(where)) == 0
    m32 = _model(metric)
    m32.store(W)
    assert m32.load(str(where)) == N_
    return m32


def _same(m, m32, q, k=10, **kw):
    Dm, Im = m.search(q, k, "", **kw)
    D32, I32 = m32.search(q, k, "", **kw)
    assert Dm.tobytes() == D32.tobytes() and Im.tobytes() == I32.tobytes()
    return Dm, Im


@pytest.mark.parametrize("metric", ["L2", "InnerProduct"], ids=["l2", "ip"])
def test_ivfflat_sq8_plugin_equals_the_oracle_and_the_fp32_model_over_w(tmp_path, metric):
    base, vmin, vmax, W, q = data(3)
    bm = METRIC[metric]
    m, cc = _indexed(base, vmin, vmax, metric, ', "raw_dtype": "SQ8", "sq8_ranges": "Trained"')      # case-insensitive
    o = _oracle(cc, metric)
    m32 = None
    B.lib().go_set_assign_mode(-1)
    try:
        assert m.add(base[:1500])
        _oracle_add(o, base[:1500], 0)
        raw = W.copy()
        o.set_raw(raw)
        D0, I0 = m.search(q, 10, "")
        compare_exact(*B.ivfflat_search(o, q, 10, P_, bm, B.make_ctx()), D0, I0)
        # an Add with a row the store refuses (NaN, inf) fails and changes nothing: no row, no key
        for poison in (np.nan, np.inf):
            bad = base[1500:].copy()
            bad[700, 7] = poison
            assert not m.add(bad)
            D1, I1 = m.search(q, 10, "")
            assert D1.tobytes() == D0.tobytes() and I1.tobytes() == I0.tobytes() and I1.max() < 1500
        assert m.add(base[1500:])              # the same vectors afterwards, at the same vids
        _oracle_add(o, base[1500:], 1500)
        m32 = _fp32_twin(m, W, tmp_path, metric)
        for n in (len(q), 5):
            Dm, Im = _same(m, m32, q[:n])
            compare_exact(*B.ivfflat_search(o, q[:n], 10, P_, bm, B.make_ctx()), Dm, Im)
        # Delete
        dead = np.unique(Im[:, :2])
        dead = dead[dead >= 0]
        assert m.delete(dead) == 0 and m32.delete(dead) == 0
        o.delete(dead)
        bmap = np.zeros((N_ + 7) // 8, np.uint8)
        np.bitwise_or.at(bmap, dead >> 3, (1 << (dead & 7)).astype(np.uint8))
        Dd, Id = _same(m, m32, q)
        compare_exact(*B.ivfflat_search(o, q, 10, P_, bm, B.make_ctx(docids_bitmap=bmap)), Dd, Id)
        assert not np.isin(Id, dead).any()
        # Update: a row the store refuses fails the Update and changes nothing
        gone = set(dead.tolist())
        live = [int(v) for v in np.random.default_rng(4).choice(N_, 40, replace=False) if int(v) not in gone]
        inf = base[live[1]].copy()
        inf[3] = -np.inf
        assert m.update(live[0], inf) != 0
        Dm, Im = _same(m, m32, q)
        assert Dm.tobytes() == Dd.tobytes() and Im.tobytes() == Id.tobytes()
        # ... and a good one moves the vector to the list of its new value (the caller's fp32 value; the twin is handed the row
        # the store holds, so only vectors that both values send to the same list serve the byte comparison)
        moved = 0
        for i, vid in enumerate(live):
            newv = base[(vid + 1000 + i) % N_].copy()
            held = S.stored(newv[None], vmin, vmax)[0]
            lno = int(B.ivfflat_assign(o, newv[None])[0])
            if lno != int(B.ivfflat_assign(o, held[None])[0]):
                continue
            assert m.update(vid, newv) == 0 and m32.update(vid, held) == 0
            raw[vid] = held
            o.update_code(lno, vid, np.zeros(1, np.uint8))
            moved += 1
        assert moved >= 12
        for n in (len(q), 5):
            Dm, Im = _same(m, m32, q[:n])
            compare_exact(*B.ivfflat_search(o, q[:n], 10, P_, bm, B.make_ctx(docids_bitmap=bmap)), Dm, Im)
    finally:
        B.lib().go_set_assign_mode(0)
        m.close()
        if m32 is not None:
            m32.close()


def test_ivfflat_sq8_plugin_dump_load(tmp_path):
    """Dump writes ivfflat.index as the fp32 model does, byte for byte, and the ranges beside it; Load sets them before the mirror
    is re-encoded from the engine's store, and fails on a missing or wrong side file and on a row the store refuses"""
    base, vmin, vmax, W, q = data(100)
    m, cc = _indexed(base, vmin, vmax)
    mb = _model()
    fresh = [_model(extra=SQ8) for _ in range(3)]
    try:
        mb.store(base)
        assert mb.set_trained(cc, np.zeros((256, D_), np.float32)) == 0
        assert m.add(base[:1500]) and m.add(base[1500:]) and mb.add(base[:1500]) and mb.add(base[1500:])
        D1, I1 = m.search(q, 10, "")
        d8, d32 = tmp_path / "sq8", tmp_path / "f32"
        d8.mkdir()
        d32.mkdir()
        assert m.dump(str(d8)) == 0 and mb.dump(str(d32)) == 0
        idx8 = [os.path.join(r, f) for r, _, fs in os.walk(d8) for f in fs if f == "ivfflat.index"]
        idx32 = [os.path.join(r, f) for r, _, fs in os.walk(d32) for f in fs if f == "ivfflat.index"]
        assert len(idx8) == 1 and len(idx32) == 1
        assert open(idx8[0], "rb").read() == open(idx32[0], "rb").read()
        side = os.path.join(os.path.dirname(idx8[0]), "raw_sq8.ranges")
        blob = open(side, "rb").read()
        assert len(blob) == 8 + 8 * D_ and blob[:4] == b"SQ8R" and struct.unpack("<i", blob[4:8])[0] == D_
        assert blob[8:8 + 4 * D_] == vmin.tobytes() and blob[8 + 4 * D_:] == vmax.tobytes()
        assert not os.path.exists(os.path.join(os.path.dirname(idx32[0]), "raw_sq8.ranges"))
        # Load into a fresh model: the same ranges, the same answers
        m2 = fresh[0]
        m2.store(base)
        assert m2.load(str(d8)) == N_
        a, b = m2.sq8_ranges()
        assert a.tobytes() == vmin.tobytes() and b.tobytes() == vmax.tobytes()
        D2, I2 = m2.search(q, 10, "")
        assert D1.tobytes() == D2.tobytes() and I1.tobytes() == I2.tobytes()
        # without the side file (the fp32 model's dump is such a directory), with the ranges of another d, with a bad magic
        m3 = fresh[1]
        m3.store(base)
        mem0 = m3.mem_bytes()
        assert m3.load(str(d32)) < 0
        other = tmp_path / "other"
        shutil.copytree(d8, other)
        with open(side.replace(str(d8), str(other)), "wb") as f:
            f.write(blob[:4] + struct.pack("<i", D_ + 1) + blob[8:] + b"\0" * 8)
        assert m3.load(str(other)) < 0
        magic = tmp_path / "magic"
        shutil.copytree(d8, magic)
        with open(side.replace(str(d8), str(magic)), "wb") as f:
            f.write(b"XXXX" + blob[4:])
        assert m3.load(str(magic)) < 0
        short = tmp_path / "short"
        shutil.copytree(d8, short)
        with open(side.replace(str(d8), str(short)), "wb") as f:
            f.write(blob[:-4])
        assert m3.load(str(short)) < 0
        assert m3.mem_bytes() == mem0 and m3.sq8_ranges() is None
        with pytest.raises(_lib.GammaHipError):      # still untrained
            m3.search(q[:4], 5, "")
        # a Load over vectors the store refuses fails before a list or a row changes (the ranges are set: they come first)
        bad = base.copy()
        bad[2345, 5] = np.nan
        m4 = fresh[2]
        m4.store(bad)
        assert m4.load(str(d8)) < 0
        with pytest.raises(_lib.GammaHipError):
            m4.search(q[:4], 5, "")
    finally:
        for mm in [m, mb] + fresh:
            mm.close()


def test_ivfflat_sq8_plugin_brute_force_and_untrained_search(tmp_path):
    """the search of an untrained model is refused (no ranges, no rows) and the model goes on to train; brute_force_search on the
    trained model goes to the flat search over sq8 rows (the model turns that switch on too): the oracle's flat search over W,
    and the fp32 twin's byte for byte"""
    base, vmin, vmax, W, q = data(7)
    m = _model(extra=SQ8)
    m32 = None
    try:
        m.store(base)
        for kw in ({}, {"brute_force": True}):
            with pytest.raises(_lib.GammaHipError):
                m.search(q[:4], 5, "", **kw)
        assert m.indexing() == 0
        a, b = m.sq8_ranges()
        assert np.array_equal(a, vmin) and np.array_equal(b, vmax)
        assert m.add(base)
        m32 = _fp32_twin(m, W, tmp_path)
        Df, If = B.flat_search(W, q, 10, B.METRIC_L2, B.make_ctx())
        compare_exact(Df, If, *_same(m, m32, q, brute_force=True))
        # ... and without the flag the trained model runs the IVFFLAT search
        cc, _ = m.trained_state(NLIST, 1)
        o = _oracle(cc, "L2")
        B.lib().go_set_assign_mode(-1)
        _oracle_add(o, base, 0)
        o.set_raw(W)
        Dm, Im = _same(m, m32, q)
        compare_exact(*B.ivfflat_search(o, q, 10, P_, B.METRIC_L2, B.make_ctx()), Dm, Im)
    finally:
        B.lib().go_set_assign_mode(0)
        m.close()
        if m32 is not None:
            m32.close()


def test_ivfflat_sq8_plugin_memory_accounting(monkeypatch):
    """GetTotalMemBytes reports rows of 1 byte per element plus the store's tables (16 bytes per dimension).  Under
    GAMMA_HIP_NO_RAW_VMM the store's capacity is max(rows needed, 1.5 x its capacity, 1024) ROWS, the same number for both models,
    and their lists are the same, so the two models differ by capacity x d x 3 bytes less the tables, n <= capacity <= 1.5 n."""
    monkeypatch.setenv("GAMMA_HIP_NO_RAW_VMM", "1")
    base, vmin, vmax, W, _ = data(5)
    mem = {}
    cc = None
    for name, extra in (("sq8", SQ8), ("f32", ', "raw_dtype": "float32"')):
        m = _model(extra=extra)
        try:
            m.store(base)
            if cc is None:
                assert m.indexing() == 0
                cc, _ = m.trained_state(NLIST, 1)
            else:
                assert m.set_trained(cc, np.zeros((256, D_), np.float32)) == 0
            for i0 in range(0, N_, 1500):
                assert m.add(base[i0:i0 + 1500])
            mem[name] = m.mem_bytes()
        finally:
            m.close()
    diff = mem["f32"] - mem["sq8"] + 16 * D_
    assert diff % (D_ * 3) == 0 and N_ * D_ * 3 <= diff <= N_ * D_ * 3 * 3 // 2, (mem, diff)


def test_ivfflat_sq8_plugin_key_rejections():
    for bad in ('"raw_dtype": "sq8"',                                                  # without the key: as before
                '"raw_dtype": "sq8", "sq8_min": -1.0, "sq8_max": 1.0',                 # HIPFLAT's form: as before
                '"raw_dtype": "sq8", "sq8_ranges": "given"',
                '"raw_dtype": "sq8", "sq8_ranges": 1',
                '"raw_dtype": "uint8", "sq8_ranges": "trained"',
                '"sq8_ranges": "trained"',
                '"raw_dtype": "sq8", "sq8_ranges": "trained", "sq8_min": -1.0, "sq8_max": 1.0'):
        with pytest.raises(_lib.GammaHipError):
            _model(extra=", " + bad)
    _model(extra=', "raw_dtype": "Sq8", "sq8_ranges": "TRAINED"').close()
    _model(extra=', "raw_dtype": "uint8"').close()
