"""GPU: the HIPIVFFLAT plugin on several devices ("devices": "0,0,0" -- every member on device 0 -- with "placement" and
"raw_placement", HIPIVFPQ's keys), driven like VectorManager drives a model.  The yardstick is the one-device HIPIVFFLAT plugin
fed the same script of Add, Search, Update, Delete, Dump and Load: byte-identical distances and labels."""
import numpy as np
import pytest

from gamma_amd import _lib
from tests import ivfflat_rows_data as R

pytestmark = pytest.mark.gpu

D_, N_, NLIST, P_ = 32, 3001, 16, 4
GROUPS = ['"devices": "0,0,0"',
          '"devices": "0,0,0", "raw_placement": "sharded"',
          '"devices": "0,0,0", "placement": "replicate"']


def data(seed):
    W = R.widened(R.base_rows(N_, D_, "uint8", seed), "uint8")      # integer-valued rows: ties included
    return W, R.centroids(W, NLIST, seed + 1), R.queries(40, D_, "uint8", seed + 2, W)


def _model(extra="", metric="L2"):
    from gamma_amd import plugin
    return plugin.PluginModel("HIPIVFFLAT", D_, '{"ncentroids": %d, "nprobe": %d, "metric_type": "%s"%s}'
                              % (NLIST, P_, metric, (", " + extra) if extra else ""), indexing_size=1500)


def _trained(cc, extra="", metric="L2"):
    m = _model(extra, metric)
    assert m.set_trained(cc, np.zeros((256, D_), np.float32)) == 0
    return m


def _same(m, one, q, k=10, **kw):
    Dm, Im = m.search(q, k, "", **kw)
    D1, I1 = one.search(q, k, "", **kw)
    assert Dm.tobytes() == D1.tobytes() and Im.tobytes() == I1.tobytes()
    return Dm, Im


@pytest.mark.parametrize("keys", GROUPS, ids=["replicated-rows", "sharded-rows", "replicate"])
def test_three_members_equal_the_one_device_plugin_through_a_script(tmp_path, keys):
    W, cc, q = data(7)
    m, one = _trained(cc, keys), _trained(cc)
    try:
        for mm in (m, one):
            mm.store(W)
            assert mm.add(W[:1500]) and mm.add(W[1500:])
        assert m.mem_bytes() > one.mem_bytes() > 0      # GetTotalMemBytes sums the members
        for n in (len(q), 5, 1):
            _same(m, one, q[:n])
        _same(m, one, q, k=10, min_score=0.0, max_score=float(np.median(one.search(q, 10, "")[0])))
        # Update (single and batched, a vid named twice), Delete
        rng = np.random.default_rng(11)
        vids = rng.choice(N_, 60, replace=False).astype(np.int64)
        vids[-1] = vids[0]
        newv = W[(vids + 1000) % N_].copy()
        for mm in (m, one):
            assert mm.update(int(vids[5]), W[3]) == 0
            assert mm.update_batch(vids, newv) == 0
        Wu = W.copy()      # the engine's store after the updates (a later entry of the batch wins)
        Wu[vids[5]] = W[3]
        for j, v in enumerate(vids):
            Wu[v] = newv[j]
        _same(m, one, np.concatenate([q, newv[:8] + 0.125]))
        dead = np.unique(one.search(q, 10, "")[1][:, :2])
        for mm in (m, one):
            assert mm.delete(dead) == 0
        Dd, Id = _same(m, one, q)
        assert not np.isin(Id, dead).any()
        # Dump and Load: each model's dump into a fresh model of the other kind
        dg, d1 = tmp_path / "group", tmp_path / "one"
        dg.mkdir()
        d1.mkdir()
        assert m.dump(str(dg)) == 0 and one.dump(str(d1)) == 0
        for extra, where in ((keys, d1), ("", dg), (keys, dg)):
            r = _model(extra)
            try:
                r.store(Wu)
                r.engine_bitmap_set(dead)
                assert r.load(str(where)) == N_
                Dr, Ir = r.search(q, 10, "")
                assert Dr.tobytes() == Dd.tobytes() and Ir.tobytes() == Id.tobytes()
            finally:
                r.close()
    finally:
        m.close()
        one.close()


def test_rejected_combinations(capfd):
    for extra in ('"devices": "0,0", "raw_dtype": "float16"',
                  '"devices": "0,0", "raw_dtype": "uint8"',
                  '"devices": "0,0", "device_filters": 1',
                  '"devices": "0,0", "placement": "replicate", "raw_placement": "sharded"',
                  '"raw_placement": "sharded"',
                  '"devices": "0,0", "placement": "elsewhere"'):
        capfd.readouterr()
        with pytest.raises(_lib.GammaHipError):
            _model(extra)
        err = capfd.readouterr().err
        assert len([l for l in err.splitlines() if l.strip()]) == 1, (extra, err)      # one log line
    # one ordinal, or no key: the one-device path
    for extra in ('"devices": "0"', '"devices": 0', ''):
        _model(extra).close()


@pytest.mark.parametrize("keys,sharded", [(GROUPS[0], False), (GROUPS[1], True)], ids=["replicated-rows", "sharded-rows"])
def test_brute_force_and_the_untrained_model(capfd, keys, sharded):
    """member 0 answers while rows are replicated; refused with an error and one log line once rows are sharded"""
    W, cc, q = data(9)
    m, one = _model(keys), _model()
    try:
        for mm in (m, one):
            mm.store(W[:1500])
        _same(m, one, q[:7])      # untrained: the flat search over the mirror (member 0's)
        for mm in (m, one):
            assert mm.set_trained(cc, np.zeros((256, D_), np.float32)) == 0
            assert mm.add(W[:1500])
        _same(m, one, q)
        if not sharded:
            _same(m, one, q[:7], brute_force=True)
        else:
            capfd.readouterr()
            with pytest.raises(_lib.GammaHipError):
                m.search(q[:7], 10, "", brute_force=True)
            err = capfd.readouterr().err
            assert len([l for l in err.splitlines() if "brute_force_search is not available" in l]) == 1, err
    finally:
        m.close()
        one.close()
