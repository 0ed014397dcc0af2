"""GPU: the HIPIVFPQ plugin with a narrow "raw_dtype" on several devices, which it serves only with "raw_placement": "sharded"
(every row once, at the device that owns its list, in 2 or 1 bytes per element).  The model is driven like
VectorManager drives one, beside the one-device plugin of the same raw_dtype: both must answer the same bytes at every step.
Every device of the group is device 0, as in tests/test_gpu_group_rawshard.py."""
import numpy as np
import pytest

from gamma_amd import _lib
from tests.parity import compare_exact
from tests.test_gpu_rawi8_plugin import D_, M_, N_, NLIST, WIDE, gauss, ints

pytestmark = pytest.mark.gpu

SHARDED = ', "devices": "0,0,0", "raw_placement": "sharded"'
UNSTORABLE = {"float16": 1e6, "uint8": 0.5, "int8": 200.0}


def _param(extra=""):
    return '{"ncentroids": %d, "nsubvector": %d, "nprobe": 8, "metric_type": "L2"%s}' % (NLIST, M_, extra)


def _model(extra, indexing_size=3000):
    from gamma_amd import plugin
    return plugin.PluginModel("HIPIVFPQ", D_, _param(extra), indexing_size=indexing_size)


def _data(dtype):
    if dtype == "float16":
        rng = np.random.default_rng(5)
        return (3.0 * rng.standard_normal((N_, D_))).astype(np.float32), (3.0 * rng.standard_normal((48, D_))).astype(np.float32)
    return ints(N_, D_, dtype, 3), gauss(48, D_, dtype, 9)


def _same(ms, q, req, **kw):
    D, I = ms[0].search(q, 10, req, **WIDE, **kw)
    Dg, Ig = ms[1].search(q, 10, req, **WIDE, **kw)
    compare_exact(D, I, Dg, Ig)
    assert D.tobytes() == Dg.tobytes() and I.tobytes() == Ig.tobytes()
    return Dg, Ig


@pytest.mark.parametrize("dtype", ["float16", "uint8", "int8"])
def test_sharded_narrow_plugin_is_the_one_device_plugin(dtype, tmp_path, capfd):
    base, q = _data(dtype)
    key = ', "raw_dtype": "%s"' % dtype
    req = '{"metric_type": "L2", "recall_num": 100, "nprobe": 8}'
    ms = [_model(key), _model(key + SHARDED)]
    try:
        for m in ms:
            m.store(base[:4500])
            # the untrained model answers by brute force over fp32 rows, which no narrow model holds: refused, as on one device
            with pytest.raises(_lib.GammaHipError):
                m.search(q[:4], 5, req, **WIDE)
            assert m.indexing() == 0
        assert [a.tobytes() for a in ms[0].trained_state(NLIST, M_)] == [a.tobytes() for a in ms[1].trained_state(NLIST, M_)]
        for m in ms:
            for i0, i1 in ((0, 3000), (3000, 3019), (3019, 4500)):
                assert m.add(base[i0:i1])
        D0, I0 = _same(ms, q, req)
        # an Add with one row the store refuses: one log line, nothing listed, no row written -- the same answers as before
        bad = base[4500:].copy()
        bad[700, 7] = UNSTORABLE[dtype]
        for m in ms:
            m.store(np.concatenate([base[:4500], bad]))
        capfd.readouterr()
        assert not ms[1].add(bad)
        lines = [l for l in capfd.readouterr().err.splitlines() if l.strip()]
        assert len(lines) == 1 and lines[0].startswith("[HIPIVFPQ]"), lines
        assert not ms[0].add(bad)
        D1, I1 = _same(ms, q, req)
        assert D1.tobytes() == D0.tobytes() and I1.tobytes() == I0.tobytes() and I1.max() < 4500
        for m in ms:
            m.store(base)
            assert m.add(base[4500:])
        for n in (len(q), 5):
            for has_rank in (True, False):
                _same(ms, q[:n], req, has_rank=has_rank)
        # brute force stays refused; the models keep serving
        for m in ms:
            with pytest.raises(_lib.GammaHipError):
                m.search(q[:4], 10, req, brute_force=True, **WIDE)
        # Update (vids named twice among them), Delete
        rng = np.random.default_rng(2)
        vids = rng.choice(N_, size=200, replace=False).astype(np.int64)
        vids = np.concatenate([vids, vids[:4]])
        vecs = base[rng.integers(0, N_, size=len(vids))].copy()
        b2 = base.copy()
        for v, x in zip(vids, vecs):
            b2[v] = x
        dead = rng.choice(N_, size=600, replace=False).astype(np.int64)
        for m in ms:
            assert m.update_batch(vids, vecs) == 0
            assert m.delete(dead) == 0
        for has_rank in (True, False):
            D, I = _same(ms, q, req, has_rank=has_rank)
            assert not np.isin(I, dead).any()
        D, I = _same(ms, q, req)
        assert ms[1].mem_bytes() > 0
        # Dump from each, Load into the other kind
        for src, extra in ((1, key), (0, key + SHARDED)):
            td = tmp_path / ("from%d" % src)
            td.mkdir()
            assert ms[src].dump(str(td)) == 0
            m2 = _model(extra)
            try:
                m2.store(b2)
                m2.engine_bitmap_set(dead)
                assert m2.load(str(td)) > 0
                Dl, Il = m2.search(q, 10, req, **WIDE)
                compare_exact(D, I, Dl, Il)
                # the loaded model goes on
                more = base[rng.integers(0, N_, size=100)].copy()
                m2.store(np.concatenate([b2, more]))
                assert m2.add(more)
                assert m2.update_batch(vids[:20], base[:20]) == 0
                m2.search(q, 10, req, **WIDE)
            finally:
                m2.close()
    finally:
        for m in ms:
            m.close()


def test_key_combinations_at_init():
    """narrow rows on several devices only where the rows are sharded; sq8 on several devices never"""
    for dtype in ("float16", "uint8", "int8", "sq8"):
        key = ', "raw_dtype": "%s"' % dtype
        for extra in (', "devices": "0,0"', ', "devices": "0,0", "raw_placement": "replicated"',
                      ', "devices": "0,0", "placement": "replicate", "raw_placement": "sharded"',
                      ', "devices": "0", "raw_placement": "sharded"'):
            with pytest.raises(_lib.GammaHipError):
                _model(key + extra)
    with pytest.raises(_lib.GammaHipError):
        _model(', "raw_dtype": "sq8"' + SHARDED)
    for dtype in ("float16", "uint8", "int8", "float32"):
        _model(', "raw_dtype": "%s"' % dtype + SHARDED).close()
        _model(', "raw_dtype": "%s", "devices": "0,0", "placement": "shard", "raw_placement": "sharded"' % dtype).close()
    from gamma_amd import plugin
    with pytest.raises(_lib.GammaHipError):        # HIPIVFFLAT: narrow rows with several devices stay rejected
        plugin.PluginModel("HIPIVFFLAT", D_, '{"ncentroids": %d, "metric_type": "L2", "raw_dtype": "uint8"%s}' % (NLIST, SHARDED),
                           indexing_size=3000)
