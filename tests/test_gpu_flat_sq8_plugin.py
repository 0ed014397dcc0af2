"""GPU: the HIPFLAT plugin with "raw_dtype": "sq8", "sq8_min", "sq8_max", driven like VectorManager drives a model (Init, Add,
Search, Update, Delete, Dump, Load).  The engine holds the fp32 rows x; the model's rows are W = sq8_ref.stored(x) under ONE
range for every dimension, and it must answer byte for byte what the fp32 HIPFLAT model fed W answers, and what the CPU oracle's
flat search over W answers.  The range is the minimum / maximum over half of the rows, so the other half clips."""
import numpy as np
import pytest

from gamma_amd import _lib
from oracle import binding as B
from tests import sq8_ref as S
from tests.parity import compare_exact

pytestmark = pytest.mark.gpu

D_, N_ = 32, 6000


def rows(n, seed, wide=1.0):
    return (np.random.default_rng(seed).standard_normal((n, D_)) * wide).astype(np.float32)


def base_and_range(seed):
    """(x, lo, hi): the second half of the rows is drawn wider than the range of the first"""
    x = np.concatenate([rows(N_ // 2, seed), rows(N_ - N_ // 2, seed + 1, wide=1.7)])
    lo, hi = float(x[:N_ // 2].min()), float(x[:N_ // 2].max())
    assert (x[N_ // 2:] < lo).any() and (x[N_ // 2:] > hi).any()
    return x, lo, hi


def stored(x, lo, hi):
    return np.ascontiguousarray(S.stored(x, np.full(D_, lo, np.float32), np.full(D_, hi, np.float32)))


def _key(lo, hi, spelled="sq8"):
    return ', "raw_dtype": "%s", "sq8_min": %r, "sq8_max": %r' % (spelled, lo, hi)


def _model(metric="L2", extra=""):
    from gamma_amd import plugin
    return plugin.PluginModel("HIPFLAT", D_, '{"metric_type": "%s"%s}' % (metric, extra))


def _same(m, m32, q, k=10):
    Dm, Im = m.search(q, k, "")
    D32, I32 = m32.search(q, k, "")
    assert Dm.tobytes() == D32.tobytes() and Im.tobytes() == I32.tobytes()
    return Dm, Im


@pytest.mark.parametrize("metric,bm", [("L2", B.METRIC_L2), ("InnerProduct", B.METRIC_IP)], ids=["l2", "ip"])
def test_flat_sq8_plugin_equals_the_fp32_model_and_the_oracle(metric, bm):
    x, lo, hi = base_and_range(3)
    W = stored(x, lo, hi)
    q = rows(80, 9)          # 80: the chunked path; q[:7]: the small path
    m, m32 = _model(metric, _key(lo, hi, "SQ8")), _model(metric)      # the value is case-insensitive
    try:
        m.store(x)
        m32.store(W)
        assert m.add(x[:3000]) and m32.add(W[:3000])
        # an Add with a row the store refuses -- a NaN -- fails and changes nothing: the model answers as before, and the same
        # vectors are added afterwards at the same vids
        D0, I0 = _same(m, m32, q)
        bad = x[3000:].copy()
        bad[1500, 7] = np.nan
        assert not m.add(bad)
        D1, I1 = _same(m, m32, q)
        assert D1.tobytes() == D0.tobytes() and I1.tobytes() == I0.tobytes() and I1.max() < 3000
        assert m.add(x[3000:]) and m32.add(W[3000:])
        for n in (len(q), 7):
            D, I = B.flat_search(W, q[:n], 10, bm, B.make_ctx())
            Dm, Im = _same(m, m32, q[:n])
            compare_exact(D, I, Dm, Im)
        # Delete
        dead = np.unique(I[:, :2])
        assert m.delete(dead) == 0 and m32.delete(dead) == 0
        bmap = np.zeros((N_ + 7) // 8, np.uint8)
        np.bitwise_or.at(bmap, dead >> 3, (1 << (dead & 7)).astype(np.uint8))
        D, I = B.flat_search(W, q, 10, bm, B.make_ctx(docids_bitmap=bmap))
        Dm, Im = _same(m, m32, q)
        compare_exact(D, I, Dm, Im)
        # Update; a row the store refuses fails the Update and changes nothing
        raw = W.copy()
        live = [int(v) for v in np.random.default_rng(4).choice(N_, 12, replace=False) if int(v) not in set(dead.tolist())]
        inf = rows(1, 999)[0]
        inf[3] = np.inf
        assert m.update(live[0], inf) != 0
        _same(m, m32, q)
        for vid in live:
            newv = rows(1, 1000 + vid, wide=1.4)[0]
            neww = stored(newv[None, :], lo, hi)[0]
            assert m.update(vid, newv) == 0 and m32.update(vid, neww) == 0
            raw[vid] = neww
        D, I = B.flat_search(raw, q, 10, bm, B.make_ctx(docids_bitmap=bmap))
        Dm, Im = _same(m, m32, q)
        compare_exact(D, I, Dm, Im)
    finally:
        m.close()
        m32.close()


def test_flat_sq8_plugin_dump_load(tmp_path):
    """Dump writes nothing for a flat model; Load mirrors the engine's vectors again, re-encoded with the range of the
    parameters -- no side file"""
    x, lo, hi = base_and_range(100)
    W = stored(x, lo, hi)
    q = rows(30, 10)
    m, m2 = _model(extra=_key(lo, hi)), _model(extra=_key(lo, hi))
    try:
        m.store(x)
        assert m.add(x)
        D1, I1 = m.search(q, 10, "")
        assert m.dump(str(tmp_path)) == 0
        m2.store(x)
        assert m2.load(str(tmp_path)) == len(x)
        D2, I2 = m2.search(q, 10, "")
        assert D1.tobytes() == D2.tobytes() and np.array_equal(I1, I2)
        compare_exact(*B.flat_search(W, q, 10, B.METRIC_L2, B.make_ctx()), D2, I2)
    finally:
        m.close()
        m2.close()
    bad = x.copy()      # a Load over vectors the store refuses fails
    bad[4321, 5] = np.nan
    m3 = _model(extra=_key(lo, hi))
    try:
        m3.store(bad)
        assert m3.load(str(tmp_path)) < 0
    finally:
        m3.close()


def test_flat_sq8_plugin_memory_accounting(monkeypatch):
    """GetTotalMemBytes counts what the handle counts: rows of one byte per element plus the decode and the encode table (4 d
    floats).  Under GAMMA_HIP_NO_RAW_VMM the store's capacity is max(rows needed, 1.5 x its capacity, 1024) ROWS, the same number
    for both models, so the fp32 model is capacity x d x 3 bytes larger less the tables, with n <= capacity <= 1.5 n."""
    monkeypatch.setenv("GAMMA_HIP_NO_RAW_VMM", "1")
    x, lo, hi = base_and_range(5)
    mem = {}
    for name, extra in (("sq8", _key(lo, hi)), ("f32", ', "raw_dtype": "float32"')):
        m = _model(extra=extra)
        try:
            m.store(x)
            for i0 in range(0, N_, 3000):
                assert m.add(x[i0:i0 + 3000])
            mem[name] = m.mem_bytes()
        finally:
            m.close()
    tables = 4 * D_ * 4
    diff = mem["f32"] - mem["sq8"] + tables
    assert diff % (3 * D_) == 0 and N_ * 3 * D_ <= diff <= N_ * 3 * D_ * 3 // 2, (mem, diff)


def test_flat_sq8_plugin_key_rejections():
    """Init fails when a key is missing, a bound is not finite as a float, sq8_min > sq8_max, or either key comes with another
    raw_dtype; a valid pair -- a constant range included -- is accepted"""
    for bad in (', "raw_dtype": "sq8"',
                ', "raw_dtype": "sq8", "sq8_min": -1',
                ', "raw_dtype": "sq8", "sq8_max": 1',
                ', "raw_dtype": "sq8", "sq8_min": "-1", "sq8_max": 1',
                ', "raw_dtype": "sq8", "sq8_min": 0, "sq8_max": 1e39',
                ', "raw_dtype": "sq8", "sq8_min": nan, "sq8_max": 1',
                ', "raw_dtype": "sq8", "sq8_min": 2, "sq8_max": 1',
                ', "raw_dtype": "uint8", "sq8_min": 0, "sq8_max": 1',
                ', "sq8_min": 0, "sq8_max": 1',
                ', "raw_dtype": "float16", "sq8_max": 1'):
        with pytest.raises(_lib.GammaHipError):
            _model(extra=bad)
    _model(extra=_key(-1.0, 1.0, "Sq8")).close()
    _model(extra=_key(0.5, 0.5)).close()
