"""GPU: the HIPIVFFLAT plugin with "raw_dtype": "float16" | "uint8" | "int8", driven like VectorManager drives a model (Init, Add,
Search, Update, Delete, Dump, Load).  The model must answer byte for byte what the fp32 HIPIVFFLAT model answers over the widened
rows W = base.astype(T).astype(float32), and what the CPU oracle's IVFFLAT search over the same lists and W answers.  Both models
are fed W, so that both assign every vector to the same list."""
import numpy as np
import pytest

from gamma_amd import _lib
from oracle import binding as B
from tests import ivfflat_rows_data as R
from tests.parity import compare_exact

pytestmark = pytest.mark.gpu

D_, N_, NLIST, P_ = 32, 3001, 16, 4
DTYPES = R.DTYPES
METRIC = {"L2": B.METRIC_L2, "InnerProduct": B.METRIC_IP}


def data(dtype, seed):
    W = R.widened(R.base_rows(N_, D_, dtype, seed), dtype)
    return W, R.centroids(W, NLIST, seed + 1), R.queries(40, D_, dtype, seed + 2, W)      # 40 x 4 pairs: list-major; q[:5]: small


def _model(metric="L2", extra=""):
    from gamma_amd import plugin
    return plugin.PluginModel("HIPIVFFLAT", D_, '{"ncentroids": %d, "nprobe": %d, "metric_type": "%s"%s}'
                              % (NLIST, P_, metric, extra), indexing_size=1500)


def _key(dtype):
    return ', "raw_dtype": "%s"' % dtype


def _trained(cc, metric="L2", extra=""):
    m = _model(metric, extra)
    assert m.set_trained(cc, np.zeros((256, D_), np.float32)) == 0
    return m


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


def _same(m, m32, q, k=10, **kw):
    Dm, Im = m.search(q, k, "", **kw)
    D32, I32 = m32.search(q, k, "", **kw)
    assert Dm.tobytes() == D32.tobytes() and Im.tobytes() == I32.tobytes()
    return Dm, Im


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("metric", ["L2", "InnerProduct"], ids=["l2", "ip"])
def test_ivfflat_plugin_equals_the_fp32_model_and_the_oracle(metric, dtype):
    W, cc, q = data(dtype, 3)
    bm = METRIC[metric]
    spelled = {"float16": "Float16", "uint8": "UInt8", "int8": "INT8"}[dtype]      # the key is case-insensitive
    m, m32 = _trained(cc, metric, _key(spelled)), _trained(cc, metric)
    o = _oracle(cc, metric)
    B.lib().go_set_assign_mode(-1)
    try:
        for mm in (m, m32):
            mm.store(W)
            assert mm.add(W[:1500])
        _oracle_add(o, W[:1500], 0)
        raw = W.copy()
        o.set_raw(raw)
        D0, I0 = _same(m, m32, q)
        compare_exact(*B.ivfflat_search(o, q, 10, P_, bm, B.make_ctx()), D0, I0)
        bad = W[1500:].copy()
        if dtype != "float16":
            bad[700, 7] += 0.5             # a row the byte store refuses: one log line ...
        else:
            bad[10, 3] = 1e6               # beyond binary16: the store's EINVAL
        assert not m.add(bad)              # ... the Add fails and changes nothing: no row, no key
        D1, I1 = _same(m, m32, q)
        assert D1.tobytes() == D0.tobytes() and I1.tobytes() == I0.tobytes() and I1.max() < 1500
        assert m.add(W[1500:]) and m32.add(W[1500:])      # the same vectors afterwards, at the same vids
        _oracle_add(o, W[1500:], 1500)
        for n in (len(q), 5):
            Dm, Im = _same(m, m32, q[:n])
            compare_exact(*B.ivfflat_search(o, q[:n], 10, P_, bm, B.make_ctx()), Dm, Im)
        # Delete
        dead = np.unique(Im[:, :2])
        assert m.delete(dead) == 0 and m32.delete(dead) == 0
        o.delete(dead)
        bmap = np.zeros((N_ + 7) // 8, np.uint8)
        np.bitwise_or.at(bmap, dead >> 3, (1 << (dead & 7)).astype(np.uint8))
        # Update: the vector moves to the list of its new value; a row a byte store refuses fails the Update and changes nothing
        live = [int(v) for v in np.random.default_rng(4).choice(N_, 12, replace=False) if int(v) not in set(dead.tolist())]
        if dtype != "float16":
            frac = W[live[1]].copy()
            frac[3] += 0.25
            assert m.update(live[0], frac) != 0
            Dm, Im = _same(m, m32, q)
            compare_exact(*B.ivfflat_search(o, q, 10, P_, bm, B.make_ctx(docids_bitmap=bmap)), Dm, Im)
        for i, vid in enumerate(live):
            newv = W[(vid + 1000 + i) % N_].copy()
            assert m.update(vid, newv) == 0 and m32.update(vid, newv) == 0
            raw[vid] = newv
            o.update_code(int(B.ivfflat_assign(o, newv[None])[0]), vid, np.zeros(1, np.uint8))
        for n in (len(q), 5):
            Dm, Im = _same(m, m32, q[:n])
            compare_exact(*B.ivfflat_search(o, q[:n], 10, P_, bm, B.make_ctx(docids_bitmap=bmap)), Dm, Im)
    finally:
        B.lib().go_set_assign_mode(0)
        m.close()
        m32.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_ivfflat_plugin_dump_load_across_row_types(tmp_path, dtype):
    """the "IvFl" file holds fp32 vectors whatever the device's rows are: a dump of the fp32 model loads into a narrow one (rows
    converted on upload) and the other way round"""
    W, cc, q = data(dtype, 100)
    d32, dn = tmp_path / "from_f32", tmp_path / "from_narrow"
    d32.mkdir()
    dn.mkdir()
    res = {}
    for extra, where in (("", d32), (_key(dtype), dn)):
        m = _trained(cc, extra=extra)
        try:
            m.store(W)
            assert m.add(W[:1500]) and m.add(W[1500:])
            res[where] = m.search(q, 10, "")
            assert m.dump(str(where)) == 0
        finally:
            m.close()
    assert res[d32][0].tobytes() == res[dn][0].tobytes() and res[d32][1].tobytes() == res[dn][1].tobytes()
    for extra, where in ((_key(dtype), d32), ("", dn)):
        m = _model(extra=extra)
        try:
            m.store(W)
            assert m.load(str(where)) == N_
            D, I = m.search(q, 10, "")
            assert D.tobytes() == res[d32][0].tobytes() and I.tobytes() == res[d32][1].tobytes()
        finally:
            m.close()
    if dtype != "float16":
        # a Load over vectors the byte store refuses fails before anything changes: no list, no row
        bad = W.copy()
        bad[2345, 5] += 0.5
        m = _model(extra=_key(dtype))
        try:
            m.store(bad)
            mem0 = m.mem_bytes()
            assert m.load(str(d32)) < 0
            assert m.mem_bytes() == mem0
        finally:
            m.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_ivfflat_plugin_brute_force_and_untrained_search(dtype):
    """HIPIVFFLAT sends brute_force_search and the search of an untrained model to the flat search: served over a narrow store
    (the model turns the flat switch on too), byte for byte the fp32 model's and the oracle's flat search over W"""
    W, cc, q = data(dtype, 7)
    m, m32 = _model(extra=_key(dtype)), _model()
    try:
        m.store(W)
        m32.store(W)
        Df, If = B.flat_search(W, q, 10, B.METRIC_L2, B.make_ctx())
        compare_exact(Df, If, *_same(m, m32, q))                 # untrained
        for mm in (m, m32):
            assert mm.set_trained(cc, np.zeros((256, D_), np.float32)) == 0
            assert mm.add(W)
        compare_exact(Df, If, *_same(m, m32, q, brute_force=True))
        # ... and without the flag the trained model runs the IVFFLAT search
        o = _oracle(cc, "L2")
        B.lib().go_set_assign_mode(-1)
        _oracle_add(o, W, 0)
        o.set_raw(W)
        compare_exact(*B.ivfflat_search(o, q, 10, P_, B.METRIC_L2, B.make_ctx()), *_same(m, m32, q))
    finally:
        B.lib().go_set_assign_mode(0)
        m.close()
        m32.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_ivfflat_plugin_memory_accounting(monkeypatch, dtype):
    """GetTotalMemBytes reports rows of 2 bytes / 1 byte per element.  Under GAMMA_HIP_NO_RAW_VMM the store's capacity is
    max(rows needed, 1.5 x its capacity, 1024) ROWS, the same number for both models, and their lists are the same, so the two
    models differ by capacity x d x (4 - elem) bytes with n <= capacity <= 1.5 n."""
    monkeypatch.setenv("GAMMA_HIP_NO_RAW_VMM", "1")
    W, cc, _ = data(dtype, 5)
    mem = {}
    for name, extra in (("narrow", _key(dtype)), ("f32", ', "raw_dtype": "float32"')):
        m = _trained(cc, extra=extra)
        try:
            m.store(W)
            for i0 in range(0, N_, 1500):
                assert m.add(W[i0:i0 + 1500])
            mem[name] = m.mem_bytes()
        finally:
            m.close()
    per_row = D_ * (4 - R.ESZ[dtype])
    diff = mem["f32"] - mem["narrow"]
    assert diff % per_row == 0 and N_ * per_row <= diff <= N_ * per_row * 3 // 2, (mem, diff)


def test_ivfflat_plugin_rejects_an_unknown_raw_dtype():
    for bad in ("uint4", "bfloat16", ""):
        with pytest.raises(_lib.GammaHipError):
            _model(extra=', "raw_dtype": "%s"' % bad)
    _model(extra=', "raw_dtype": "Float32"').close()
