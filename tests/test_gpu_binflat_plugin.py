"""GPU: HIPBINARYIVF's exact search (gamma_amd/host/gamma_index_binivf_hip.cc: brute_force_search, and every search of a
model that is not trained yet) through the binary harness, against the one-list yardstick (tests/binflat_ref.py) over the
rows the ENGINE'S STORE holds -- strict at every rank."""
import numpy as np
import pytest

from gamma_amd import plugin
from tests import binflat_ref as BF
from tests import binivf_ref as BR

pytestmark = pytest.mark.gpu


def _same(D, I, Dr, Ir):
    assert np.array_equal(I, Ir) and D.tobytes() == Dr.tobytes()


def _model(nbits, nlist, indexing_size, codes, params=None):
    m = plugin.BinaryPluginModel("HIPBINARYIVF", nbits // 8, params if params is not None else '{"ncentroids": %d}' % nlist,
                                 indexing_size)
    m.store(codes)
    return m


def test_untrained_model_answers_exactly():
    nbits, nlist = 128, 16
    codes = BR.clustered_codes(9000, nbits, 10, flip=0.03, seed=3, dup_frac=0.2)
    x = np.ascontiguousarray(np.concatenate([codes[::301], BR.clustered_codes(10, nbits, 4, seed=9)]))
    dm = BF.hamming_matrix(x, codes)
    m = _model(nbits, nlist, 100000, codes[:5000])
    try:
        assert m.state()["trained"] == 0
        mem0 = m.mem_bytes()
        for k in (1, 10, 100):
            rc, D, I = m.search(x, k, "", 0, 1e4)
            assert rc == 0
            _same(D, I, *BF.search(dm[:, :5000], k, 0, 1e4))
        assert m.mem_bytes() - mem0 >= 5000 * nbits // 8   # the mirror is counted
        rc, D, I = m.search(x, 10)   # the default window
        assert rc == 0
        _same(D, I, *BF.search(dm[:, :5000], 10))
        m.store(codes[5000:])   # more rows in the engine's store: the next search sees them
        for brute in (False, True):
            rc, D, I = m.search(x, 10, '{"nprobe": 3}', 0, 1e4, brute=brute)
            assert rc == 0
            _same(D, I, *BF.search(dm, 10, 0, 1e4))
        assert m.state()["trained"] == 0
    finally:
        m.close()


def test_trained_model_brute_force_covers_rows_not_yet_added():
    nbits, nlist = 128, 16
    n = 7000
    codes = BR.clustered_codes(n, nbits, 10, flip=0.03, seed=7, dup_frac=0.2)
    x = np.ascontiguousarray(np.concatenate([codes[::131], BR.clustered_codes(20, nbits, 4, seed=9)]))
    dm = BF.hamming_matrix(x, codes)
    m = _model(nbits, nlist, n, codes)
    try:
        assert m.indexing() == 0
        assert m.add(codes[:5000])   # 2000 rows are stored but not in the lists yet
        cc = BR.train(codes[:nlist * 256], nlist)
        lists = BR.assign_lists(codes[:5000], cc)
        before = m.search(x, 10, '{"nprobe": 8}', 0, 1e4)
        assert before[0] == 0
        _same(before[1], before[2], *BR.search(lists, cc, x, 10, 8, 0, 1e4))
        mem0 = m.mem_bytes()
        for k in (10, 100):
            rc, D, I = m.search(x, k, '{"nprobe": 8}', 0, 1e4, brute=True)
            assert rc == 0
            _same(D, I, *BF.search(dm, k, 0, 1e4))   # ALL stored rows, nprobe ignored
        assert m.mem_bytes() - mem0 >= n * nbits // 8
        after = m.search(x, 10, '{"nprobe": 8}', 0, 1e4)   # the ordinary search is what it was
        assert after[0] == 0 and np.array_equal(after[2], before[2]) and after[1].tobytes() == before[1].tobytes()
        # deletes and range results (incl. NOT) through the engine's bitmap, both paths
        deleted = np.arange(0, n, 11)
        assert m.delete(deleted) == 0
        r1 = np.random.default_rng(3).choice(n, 2500, replace=False)
        for ranges in (None, [(r1, False)], [(np.arange(100, 3000), True)], [(r1, False), (np.arange(500, 900), True)]):
            f = BR.Filter(deleted=deleted, ranges=ranges)
            rc, D, I = m.search(x, 20, "", 0, 1e4, ranges=ranges, brute=True)
            assert rc == 0
            _same(D, I, *BF.search(dm, 20, 0, 1e4, filt=f))
            rc, D, I = m.search(x, 20, '{"nprobe": 8}', 0, 1e4, ranges=ranges)
            assert rc == 0
            _same(D, I, *BR.search(lists, cc, x, 20, 8, 0, 1e4, filt=f))
        rc, D, I = m.search(x, 5, "", 1e5, 2e5, brute=True)   # empty slots
        assert rc == 0 and (I == -1).all() and (D == np.float32(2147483648.0)).all()
        rc, _, _ = m.search(x, 5000, "", 0, 1e4, brute=True)   # k beyond the replay's heap: the ABI's rc
        assert rc == -6
    finally:
        m.close()
