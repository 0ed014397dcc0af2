"""GPU: the HIPFLAT plugin with "raw_dtype": "float16" | "uint8" | "int8", driven like VectorManager drives a model (Init, Add,
Search, Update, Delete, Dump, Load).  The model must answer byte for byte what the fp32 HIPFLAT model answers over the widened
rows W = base.astype(T).astype(float32), and what the CPU oracle's flat search over W answers."""
import numpy as np
import pytest

from gamma_amd import _lib
from oracle import binding as B
from tests.parity import compare_exact

pytestmark = pytest.mark.gpu

D_, N_ = 32, 6000
DTYPES = ["float16", "uint8", "int8"]
NP = {"float16": np.float16, "uint8": np.uint8, "int8": np.int8}
RANGE = {"uint8": (0, 255), "int8": (-128, 127)}
ESZ = {"float16": 2, "uint8": 1, "int8": 1}


def rows(n, dtype, seed):
    """rows the store of this type holds exactly"""
    rng = np.random.default_rng(seed)
    if dtype == "float16":
        return (rng.standard_normal((n, D_)) * 3).astype(np.float16).astype(np.float32)
    lo, hi = RANGE[dtype]
    x = rng.integers(lo, hi + 1, size=(n, D_)).astype(np.float32)
    x[0, 0], x[0, -1] = lo, hi
    return x


def queries(n, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == "float16":
        return (rng.standard_normal((n, D_)) * 3).astype(np.float32)
    lo, hi = RANGE[dtype]
    return ((lo + hi) / 2.0 + 60.0 * rng.standard_normal((n, D_))).astype(np.float32)


def _model(metric="L2", extra=""):
    from gamma_amd import plugin
    return plugin.PluginModel("HIPFLAT", D_, '{"metric_type": "%s"%s}' % (metric, extra))


def _key(dtype):
    return ', "raw_dtype": "%s"' % dtype


def _same(m, m32, q, k=10):
    Dm, Im = m.search(q, k, "")
    D32, I32 = m32.search(q, k, "")
    assert Dm.tobytes() == D32.tobytes() and Im.tobytes() == I32.tobytes()
    return Dm, Im


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("metric,bm", [("L2", B.METRIC_L2), ("InnerProduct", B.METRIC_IP)], ids=["l2", "ip"])
def test_flat_plugin_equals_the_fp32_model_and_the_oracle(metric, bm, dtype):
    W = rows(N_, dtype, 3)
    q = queries(80, dtype, 9)          # 80: the chunked path; q[:7]: the small path
    spelled = {"float16": "Float16", "uint8": "UInt8", "int8": "INT8"}[dtype]      # the key is case-insensitive
    m, m32 = _model(metric, _key(spelled)), _model(metric)
    try:
        for mm in (m, m32):
            mm.store(W)
            assert mm.add(W[:3000])
        if dtype != "float16":
            # an Add with a row the store refuses fails and changes nothing: the model answers as before, and the same
            # vectors are added afterwards at the same vids
            D0, I0 = _same(m, m32, q)
            bad = W[3000:].copy()
            bad[1500, 7] += 0.5
            assert not m.add(bad)
            D1, I1 = _same(m, m32, q)
            assert D1.tobytes() == D0.tobytes() and I1.tobytes() == I0.tobytes() and I1.max() < 3000
        else:
            big = W[3000:].copy()
            big[10, 3] = 1e6               # beyond binary16: the store's EINVAL
            assert not m.add(big)
        assert m.add(W[3000:]) and m32.add(W[3000:])
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
        # Update; a row a byte store refuses fails the Update and changes nothing
        raw = W.copy()
        live = [int(v) for v in np.random.default_rng(4).choice(N_, 12, replace=False) if int(v) not in set(dead.tolist())]
        if dtype != "float16":
            frac = rows(1, dtype, 999)[0]
            frac[3] += 0.25
            assert m.update(live[0], frac) != 0
            _same(m, m32, q)
        for vid in live:
            newv = rows(2, dtype, 1000 + vid)[1]
            assert m.update(vid, newv) == 0 and m32.update(vid, newv) == 0
            raw[vid] = newv
        D, I = B.flat_search(raw, q, 10, bm, B.make_ctx(docids_bitmap=bmap))
        Dm, Im = _same(m, m32, q)
        compare_exact(D, I, Dm, Im)
    finally:
        m.close()
        m32.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_flat_plugin_dump_load(tmp_path, dtype):
    """Dump writes nothing for a flat model; Load mirrors the engine's vectors again, converted on upload"""
    W = rows(N_, dtype, 100)
    q = queries(30, dtype, 10)
    m, m2 = _model(extra=_key(dtype)), _model(extra=_key(dtype))
    try:
        m.store(W)
        assert m.add(W)
        D1, I1 = m.search(q, 10, "")
        assert m.dump(str(tmp_path)) == 0
        m2.store(W)
        assert m2.load(str(tmp_path)) == len(W)
        D2, I2 = m2.search(q, 10, "")
        assert D1.tobytes() == D2.tobytes() and np.array_equal(I1, I2)
        compare_exact(*B.flat_search(W, q, 10, B.METRIC_L2, B.make_ctx()), D2, I2)
    finally:
        m.close()
        m2.close()
    if dtype != "float16":      # a Load over vectors the byte store refuses fails
        bad = W.copy()
        bad[4321, 5] += 0.5
        m3 = _model(extra=_key(dtype))
        try:
            m3.store(bad)
            assert m3.load(str(tmp_path)) < 0
        finally:
            m3.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_flat_plugin_memory_accounting(monkeypatch, dtype):
    """GetTotalMemBytes reports rows of 2 bytes / 1 byte per element.  Under GAMMA_HIP_NO_RAW_VMM the store's capacity is
    max(rows needed, 1.5 x its capacity, 1024) ROWS, the same number for both models, so the two models differ by
    capacity x d x (4 - elem) bytes with n <= capacity <= 1.5 n."""
    monkeypatch.setenv("GAMMA_HIP_NO_RAW_VMM", "1")
    W = rows(N_, dtype, 5)
    mem = {}
    for name, extra in (("narrow", _key(dtype)), ("f32", ', "raw_dtype": "float32"')):
        m = _model(extra=extra)
        try:
            m.store(W)
            for i0 in range(0, N_, 3000):
                assert m.add(W[i0:i0 + 3000])
            mem[name] = m.mem_bytes()
        finally:
            m.close()
    per_row = D_ * (4 - ESZ[dtype])
    diff = mem["f32"] - mem["narrow"]
    assert diff % per_row == 0 and N_ * per_row <= diff <= N_ * per_row * 3 // 2, (mem, diff)


def test_flat_plugin_rejects_an_unknown_raw_dtype():
    for bad in ("uint4", "bfloat16", ""):
        with pytest.raises(_lib.GammaHipError):
            _model(extra=', "raw_dtype": "%s"' % bad)
    _model(extra=', "raw_dtype": "Float32"').close()
