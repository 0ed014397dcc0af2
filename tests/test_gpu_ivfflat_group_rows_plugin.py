"""GPU: the HIPIVFFLAT plugin on several devices with a narrow "raw_dtype" behind "group_rows": "raw_dtype"  --
"devices": "0,0,0", every member on device 0, in the three placements the fp32 group takes -- driven like VectorManager drives a
model.  The yardstick is the one-device HIPIVFFLAT plugin of the same raw_dtype fed the same script of Add, Search, Update,
Delete, Dump and Load: byte-identical distances and labels at every step."""
import numpy as np
import pytest

from gamma_amd import _lib
from tests import ivfflat_rows_data as R

pytestmark = pytest.mark.gpu

D_, N_, NLIST, P_ = 32, 3001, 16, 4
KEY = '"group_rows": "raw_dtype"'
GROUPS = ['"devices": "0,0,0"',
          '"devices": "0,0,0", "raw_placement": "sharded"',
          '"devices": "0,0,0", "placement": "replicate"']
IDS = ["replicated-rows", "sharded-rows", "replicate"]
UNSTORABLE = {"uint8": 0.5, "int8": 200.0}      # (float16: where the rows are sharded, HIPIVFPQ's range rule)
DTYPE = pytest.mark.parametrize("dtype", R.DTYPES)


def data(dtype, seed):
    """what the engine's store holds (fp32; the float16 rows do not survive the store unchanged), centroids, queries"""
    base = R.base_rows(N_, D_, dtype, seed)
    W = R.widened(base, dtype)
    return base, R.centroids(W, NLIST, seed + 1), R.queries(40, D_, dtype, seed + 2, W)


def _model(extra="", metric="L2"):
    from gamma_amd import plugin
    return plugin.PluginModel("HIPIVFFLAT", D_, '{"ncentroids": %d, "nprobe": %d, "metric_type": "%s"%s}'
                              % (NLIST, P_, metric, (", " + extra) if extra else ""), indexing_size=1500)


def _dt(dtype):
    return '"raw_dtype": "%s"' % dtype


def _group(dtype, keys):
    return "%s, %s, %s" % (_dt(dtype), keys, KEY)


def _trained(cc, extra):
    m = _model(extra)
    assert m.set_trained(cc, np.zeros((256, D_), np.float32)) == 0
    return m


def _same(m, one, q, k=10, **kw):
    Dm, Im = m.search(q, k, "", **kw)
    D1, I1 = one.search(q, k, "", **kw)
    assert Dm.tobytes() == D1.tobytes() and Im.tobytes() == I1.tobytes()
    return Dm, Im


@pytest.mark.parametrize("keys", GROUPS, ids=IDS)
@DTYPE
def test_three_narrow_members_equal_the_one_device_plugin_through_a_script(tmp_path, capfd, dtype, keys):
    base, cc, q = data(dtype, 7)
    m, one = _trained(cc, _group(dtype, keys)), _trained(cc, _dt(dtype))
    try:
        for mm in (m, one):
            mm.store(base)
            assert mm.add(base[:1500]) and mm.add(base[1500:2900])
        assert m.mem_bytes() > 0 and one.mem_bytes() > 0
        for n in (len(q), 5, 1):
            _same(m, one, q[:n])
        D0, I0 = _same(m, one, q, k=10, min_score=0.0, max_score=float(np.median(one.search(q, 10, "")[0])))
        # an Add with a row the store refuses: one log line, both models answer as before
        sharded = "sharded" in keys
        if dtype in UNSTORABLE or sharded:
            bad = base[2900:].copy()
            bad[50, 7] = UNSTORABLE.get(dtype, 1e6)
            Da, Ia = _same(m, one, q)
            for mm in (m, one):
                mm.store(np.concatenate([base[:2900], bad]))
            capfd.readouterr()
            assert not m.add(bad)
            lines = [l for l in capfd.readouterr().err.splitlines() if l.strip()]
            assert len(lines) == 1 and "refused" in lines[0], lines
            if dtype in UNSTORABLE:
                assert not one.add(bad)
            Db, Ib = m.search(q, 10, "")
            assert Db.tobytes() == Da.tobytes() and Ib.tobytes() == Ia.tobytes() and Ib.max() < 2900
            if dtype in UNSTORABLE:
                _same(m, one, q)
        for mm in (m, one):
            mm.store(base)
            assert mm.add(base[2900:])
        _same(m, one, q)
        # Update (single and batched, a vid named twice), Delete
        rng = np.random.default_rng(11)
        vids = rng.choice(N_, 60, replace=False).astype(np.int64)
        vids[-1] = vids[0]
        newv = base[(vids + 1000) % N_].copy()
        for mm in (m, one):
            assert mm.update(int(vids[5]), base[3]) == 0
            assert mm.update_batch(vids, newv) == 0
        Bu = base.copy()      # the engine's store after the updates (a later entry of the batch wins)
        Bu[vids[5]] = base[3]
        for j, v in enumerate(vids):
            Bu[v] = newv[j]
        _same(m, one, np.concatenate([q, R.widened(newv[:8], dtype) + 0.125]))
        dead = np.unique(one.search(q, 10, "")[1][:, :2])
        for mm in (m, one):
            assert mm.delete(dead) == 0
        Dd, Id = _same(m, one, q)
        assert not np.isin(Id, dead).any()
        # Dump and Load: each model's dump into a fresh model of the other kind, and the group's into a group
        dg, d1 = tmp_path / "group", tmp_path / "one"
        dg.mkdir()
        d1.mkdir()
        assert m.dump(str(dg)) == 0 and one.dump(str(d1)) == 0
        for extra, where in ((_group(dtype, keys), d1), (_dt(dtype), dg), (_group(dtype, keys), dg)):
            r = _model(extra)
            try:
                r.store(Bu)
                r.engine_bitmap_set(dead)
                assert r.load(str(where)) == N_
                Dr, Ir = r.search(q, 10, "")
                assert Dr.tobytes() == Dd.tobytes() and Ir.tobytes() == Id.tobytes()
            finally:
                r.close()
    finally:
        m.close()
        one.close()


@pytest.mark.parametrize("dtype", ["uint8", "int8"])
def test_a_load_that_meets_a_row_the_store_cannot_hold_fails(tmp_path, dtype):
    base, cc, q = data(dtype, 7)
    keys = _group(dtype, GROUPS[1])
    m = _trained(cc, keys)
    try:
        m.store(base)
        assert m.add(base)
        assert m.dump(str(tmp_path)) == 0
    finally:
        m.close()
    for extra in (keys, _dt(dtype)):      # the group as the one-device narrow model
        r = _model(extra)
        try:
            bad = base.copy()
            bad[700, 7] = UNSTORABLE[dtype]
            r.store(bad)
            assert r.load(str(tmp_path)) < 0
        finally:
            r.close()


@pytest.mark.parametrize("keys,sharded", [(GROUPS[0], False), (GROUPS[1], True)], ids=["replicated-rows", "sharded-rows"])
@DTYPE
def test_brute_force_and_the_untrained_model(capfd, dtype, keys, sharded):
    """member 0 answers from its narrow mirror while rows are replicated, or until the first Add after training; refused with an
    error and one log line once rows are sharded"""
    base, cc, q = data(dtype, 9)
    m, one = _model(_group(dtype, keys)), _model(_dt(dtype))
    try:
        for mm in (m, one):
            mm.store(base[:1500])
        _same(m, one, q[:7])      # untrained: the flat search over the narrow mirror (member 0's)
        for mm in (m, one):
            assert mm.set_trained(cc, np.zeros((256, D_), np.float32)) == 0
        _same(m, one, q[:7], brute_force=True)      # trained, nothing added yet: the rows are not sharded yet
        for mm in (m, one):
            assert mm.add(base[:1500])
        _same(m, one, q)
        if not sharded:
            _same(m, one, q[:7], brute_force=True)
        else:
            capfd.readouterr()
            with pytest.raises(_lib.GammaHipError):
                m.search(q[:7], 10, "", brute_force=True)
            err = capfd.readouterr().err
            assert len([l for l in err.splitlines() if "brute_force_search is not available" in l]) == 1, err
            _same(m, one, q)      # the model keeps serving
    finally:
        m.close()
        one.close()


def test_sharded_uint8_members_take_less_memory_than_sharded_fp32_members():
    """GetTotalMemBytes sums the members, and the store grows in chunks of 64 MB: 48000 rows of 1024 elements over two members are
    94 MB of fp32 each (two chunks) and 23 MB of uint8 (one)"""
    d, n = 1024, 48000
    rng = np.random.default_rng(4)
    big = rng.integers(0, 256, size=(n // 16, d)).astype(np.float32).repeat(16, axis=0)
    ccb = np.ascontiguousarray(big[:: n // NLIST][:NLIST] + 0.25)
    sharded2 = '"devices": "0,0", "raw_placement": "sharded"'
    from gamma_amd import plugin
    mem = {}
    for name, extra in (("uint8", '"raw_dtype": "uint8", %s, %s' % (sharded2, KEY)), ("float32", sharded2)):
        m = plugin.PluginModel("HIPIVFFLAT", d, '{"ncentroids": %d, "nprobe": %d, "metric_type": "L2", %s}' % (NLIST, P_, extra),
                               indexing_size=1500)
        try:
            assert m.set_trained(ccb, np.zeros((256, d), np.float32)) == 0
            m.store(big)
            assert m.add(big)
            mem[name] = m.mem_bytes()
        finally:
            m.close()
    assert 0 < mem["uint8"] < mem["float32"], mem


def test_rejected_combinations(capfd):
    for extra in ('"devices": "0,0", "raw_dtype": "uint8", "group_rows": "uint8"',
                  '"devices": "0,0", "raw_dtype": "uint8", "group_rows": "float32"',
                  '"raw_dtype": "uint8", %s' % KEY,
                  '"devices": "0", "raw_dtype": "float16", %s' % KEY,
                  '"devices": "0,0", "raw_dtype": "sq8", "sq8_ranges": "trained", %s' % KEY,
                  '"devices": "0,0", "raw_dtype": "int8", "device_filters": 1, %s' % KEY,
                  '"devices": "0,0", "raw_dtype": "float16"',
                  '"devices": "0,0", "raw_dtype": "uint8"',
                  '"raw_dtype": "uint8", "devices": "0,0,0", "raw_placement": "sharded"'):
        capfd.readouterr()
        with pytest.raises(_lib.GammaHipError):
            _model(extra)
        err = capfd.readouterr().err
        assert len([l for l in err.splitlines() if l.strip()]) == 1, (extra, err)      # one log line
    # accepted: the key beside float32 rows means nothing
    _model('"devices": "0,0", %s' % KEY).close()
    _model('"devices": "0,0", "raw_dtype": "float32", "raw_placement": "sharded", %s' % KEY).close()
