"""GPU: the HIPBINARYIVF RetrievalModel plugin (gamma_amd/host/gamma_index_binivf_hip.cc) driven through the binary harness
(gamma_amd/host/harness_binary.cc) the way VectorManager drives a model over a BINARY store, against the restatement
(tests/binivf_ref.py): Init's parameters, the training-size rule of Indexing, the nprobe rules of Parse / Search, the score
window, filters, Update / Dump / Load as the reference's no-ops, the empty-slot padding -- results strict at every rank."""
import numpy as np
import pytest

from gamma_amd import plugin
from tests import binivf_ref as BR

pytestmark = pytest.mark.gpu


def _same(D, I, Dr, Ir):
    assert np.array_equal(I, Ir) and D.tobytes() == Dr.tobytes()


def _model(nbits, nlist, indexing_size, codes, params=None):
    m = plugin.BinaryPluginModel("HIPBINARYIVF", nbits // 8, params if params is not None else '{"ncentroids": %d}' % nlist,
                                 indexing_size)
    m.store(codes)
    return m


def test_registered_and_init_parameters():
    assert plugin.load_host().gh_model_registered(b"HIPBINARYIVF") == 1
    m = plugin.BinaryPluginModel("HIPBINARYIVF", 16, "", 1000)
    try:
        # BinaryModelParams: ncentroids default 256; the model's nprobe is 20 whatever the parameters say
        assert m.state() == {"nlist": 256, "nprobe": 20, "nbits": 128, "trained": 0}
    finally:
        m.close()
    m = plugin.BinaryPluginModel("HIPBINARYIVF", 8, '{"ncentroids": 32, "nprobe": 7}', 1000)
    try:
        assert m.state() == {"nlist": 32, "nprobe": 20, "nbits": 64, "trained": 0}
    finally:
        m.close()
    with pytest.raises(Exception):
        plugin.BinaryPluginModel("HIPBINARYIVF", 8, '{"ncentroids": 0}', 1000)


@pytest.mark.parametrize("indexing_size,num", [(10, 16 * 39), (700, 700), (100000, 16 * 256)])
def test_training_size_rule(indexing_size, num):
    nbits, nlist = 64, 16
    codes = BR.clustered_codes(5000, nbits, 8, flip=0.03, seed=indexing_size, dup_frac=0.2)
    m = _model(nbits, nlist, indexing_size, codes[:num - 1])
    try:
        assert not m.add(codes[:10])   # Add before training
        assert m.indexing() == -1      # the store holds fewer vectors than num
        m.store(codes[num - 1:])
        assert m.indexing() == 0 and m.state()["trained"] == 1
        assert m.add(codes)
        cc = BR.train(codes[:num], nlist)   # trained on the first num vectors of the store
        lists = BR.assign_lists(codes, cc)
        x = codes[::97]
        rc, D, I = m.search(x, 10, '{"nprobe": 16}', 0, 1e4)
        assert rc == 0
        _same(D, I, *BR.search(lists, cc, x, 10, 16, 0, 1e4))
    finally:
        m.close()


def test_search_contract():
    nbits, nlist = 128, 16
    n = 6000
    codes = BR.clustered_codes(n, nbits, 10, flip=0.03, seed=7, dup_frac=0.2)
    m = _model(nbits, nlist, n, codes)
    try:
        assert m.indexing() == 0
        assert m.add(codes[:2500]) and m.add(codes[2500:])
        cc = BR.train(codes[:nlist * 256], nlist)   # indexing_size > nlist * 256: the first nlist * 256 vectors
        lists = BR.assign_lists(codes, cc)
        x = np.concatenate([codes[::131], BR.clustered_codes(20, nbits, 4, seed=9)])
        # nprobe: the request's when in (0, nlist], else 20 (more than nlist: the extra probe slots are empty)
        for params, P in (("", 20), ('{"nprobe": 3}', 3), ('{"nprobe": 16}', 16), ('{"nprobe": 17}', 20),
                          ('{"nprobe": 0}', 20), ('{"nprobe": -4}', 20)):
            for k in (1, 10, 100):
                rc, D, I = m.search(x, k, params)
                assert rc == 0
                _same(D, I, *BR.search(lists, cc, x, k, P))
        # the default window [FLT_MIN, FLT_MAX] excludes an exact duplicate, [0, 1e4] keeps it
        rc, D, _ = m.search(codes[:30], 3, '{"nprobe": 16}')
        assert (D > 0).all()
        rc, D, _ = m.search(codes[:30], 3, '{"nprobe": 16}', 0, 1e4)
        assert (D[:, 0] == 0).all()
        # range results (incl. NOT) and deletes through the engine's bitmap
        deleted = np.arange(0, n, 11)
        assert m.delete(deleted) == 0
        r1 = np.random.default_rng(3).choice(n, 2000, replace=False)
        for ranges in (None, [(r1, False)], [(np.arange(100, 3000), True)], [(r1, False), (np.arange(500, 900), True)]):
            f = BR.Filter(deleted=deleted, ranges=ranges)
            rc, D, I = m.search(x, 20, '{"nprobe": 8}', 0, 1e4, ranges=ranges)
            assert rc == 0
            _same(D, I, *BR.search(lists, cc, x, 20, 8, 0, 1e4, filt=f))
        # empty slots: (float)INT32_MAX and -1
        rc, D, I = m.search(x, 5, '{"nprobe": 16}', 1e5, 2e5)
        assert rc == 0 and (I == -1).all() and (D == np.float32(2147483648.0)).all()
        # Update, Dump and Load are the reference's no-ops: 0, and the index is what it was
        before = m.search(x, 10, '{"nprobe": 16}', 0, 1e4)
        assert m.update(5, np.full(nbits // 8, 0xff, np.uint8)) == 0
        assert m.dump("/nonexistent/dir") == 0 and m.load("/nonexistent/dir") == 0
        after = m.search(x, 10, '{"nprobe": 16}', 0, 1e4)
        assert np.array_equal(before[2], after[2]) and before[1].tobytes() == after[1].tobytes()
        assert m.mem_bytes() > 0
    finally:
        m.close()
