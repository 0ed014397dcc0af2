"""GPU: the binary IVF model (gamma_hip_binivf_*) against its restatement (tests/binivf_ref.py), strictly: centroid codes
byte for byte, probes, and labels + distances equal at every rank -- inside the exact ties that Hamming distances make
at nearly every k-th place too."""
import numpy as np
import pytest
import torch

from gamma_amd import api
from tests import binivf_ref as BR

pytestmark = pytest.mark.gpu


def _args(nprobe, lo=None, hi=None, **kw):
    return api.SearchArgs(nprobe=nprobe, min_score=lo, max_score=hi, **kw)


def _same(D, I, Dr, Ir, what=""):
    assert I.shape == Ir.shape
    bad = np.nonzero((I != Ir).any(axis=1) | (D.view(np.uint32) != Dr.view(np.uint32)).any(axis=1))[0]
    assert bad.size == 0, "%s: %d rows differ, first %d: dev %s %s ref %s %s" % (
        what, bad.size, bad[0], D[bad[0]][:8], I[bad[0]][:8], Dr[bad[0]][:8], Ir[bad[0]][:8])


def _index(nbits, nlist, base, cc, bucket_init=1000):
    g = api.GammaHip(0)
    g.binivf_init(nbits, nlist, bucket_init_size=bucket_init)
    g.binivf_set_trained(cc)
    g.binivf_add(base, 0)
    return g


def _queries(base, n, nbits, seed):
    rng = np.random.default_rng(seed)
    half = n // 2
    new = BR.clustered_codes(n - half, nbits, 16, flip=0.08, seed=seed + 1, dup_frac=0.0)
    return np.ascontiguousarray(np.concatenate([base[rng.integers(0, base.shape[0], half)], new]))


@pytest.mark.parametrize("nbits,nlist", [(64, 16), (256, 16), (512, 16), (256, 64)])
def test_training_is_byte_identical(nbits, nlist):
    n = nlist * 60
    codes = BR.clustered_codes(n, nbits, max(2, nlist // 2), flip=0.03, seed=nbits + nlist, dup_frac=0.2)
    g = api.GammaHip(0)
    try:
        assert np.array_equal(g.binivf_train(codes, nlist), BR.train(codes, nlist))
        eq = codes[:nlist].copy()   # n == nlist: the copy path
        assert np.array_equal(g.binivf_train(eq, nlist), BR.train(eq, nlist))
    finally:
        g.close()


@pytest.mark.parametrize("nbits,nlist", [(64, 8), (200, 32), (1024, 16)])
def test_coarse_probes(nbits, nlist):
    base = BR.clustered_codes(2000, nbits, 8, seed=nbits)
    cc = base[:nlist].copy()
    g = _index(nbits, nlist, base, cc)
    try:
        x = _queries(base, 100, nbits, 7)
        for k in (1, 5, nlist, 20 if nlist < 20 else nlist + 3):
            D, I = g.binivf_assign(x, k)
            Dr, Ir = BR.coarse(x, cc, k)
            assert np.array_equal(I, Ir) and np.array_equal(D, Dr), k
        for l in range(nlist):   # Add = assign (k = 1) + AddKeys in vid order
            ids, codes = g.get_list(l)
            rv, rc = BR.assign_lists(base, cc)[l]
            assert np.array_equal(ids, rv) and np.array_equal(codes, rc)
    finally:
        g.close()


@pytest.mark.parametrize("nbits", [32, 64, 200, 256, 512, 1024])
def test_search_grid(nbits):
    nlist = 32
    base = BR.clustered_codes(6000, nbits, 24, flip=0.04, seed=nbits, dup_frac=0.1)
    cc = BR.train(base[:nlist * 40], nlist)
    lists = BR.assign_lists(base, cc)
    g = _index(nbits, nlist, base, cc)
    try:
        x = _queries(base, 64, nbits, nbits + 1)
        for k in (1, 10, 100, 1000):
            for nprobe in (1, 20, nlist):
                for nq in (1, 7, 64):
                    D, I = g.binivf_search(x[:nq], k, _args(nprobe))
                    Dr, Ir = BR.search(lists, cc, x[:nq], k, nprobe)
                    _same(D, I, Dr, Ir, "nbits %d k %d nprobe %d nq %d" % (nbits, k, nprobe, nq))
        xl = _queries(base, 1000, nbits, nbits + 2)
        for k in (10, 1000):
            for nprobe in (1, nlist):
                D, I = g.binivf_search(xl, k, _args(nprobe))
                Dr, Ir = BR.search(lists, cc, xl, k, nprobe)
                _same(D, I, Dr, Ir, "nbits %d k %d nprobe %d nq 1000" % (nbits, k, nprobe))
    finally:
        g.close()


@pytest.mark.parametrize("nbits,nlist", [(256, 256), (256, 1024), (1024, 512), (40, 300)])
def test_coarse_and_search_at_realistic_nlist(nbits, nlist):
    """the coarse walk over many 64-centroid blocks (HeapWalk's sifts in flight across blocks), the centroids in LDS
    (256 x 32 B, 1024 x 32 B) and read through L2 (512 x 128 B: beyond the 64 KB of centroids + heap), nprobe and k > 64"""
    n = max(20 * nlist, 20000)
    base = BR.clustered_codes(n, nbits, nlist // 2, flip=0.04, seed=nbits + nlist, dup_frac=0.1)
    cc = base[np.random.default_rng(nlist).choice(n, nlist, replace=False)].copy()
    lists = BR.assign_lists(base, cc)
    g = _index(nbits, nlist, base, cc)
    try:
        for l in range(0, nlist, max(1, nlist // 64)):   # Add's assignment
            ids, codes = g.get_list(l)
            assert np.array_equal(ids, lists[l][0]) and np.array_equal(codes, lists[l][1]), l
        x = _queries(base, 200, nbits, nlist + 5)
        for k in (1, 20, 100, 300):
            D, I = g.binivf_assign(x, k)
            Dr, Ir = BR.coarse(x, cc, k)
            assert np.array_equal(I, Ir) and np.array_equal(D, Dr), k
        for k, nprobe in ((10, 20), (100, 100), (1, 256), (300, 70)):
            D, I = g.binivf_search(x, k, _args(nprobe))
            Dr, Ir = BR.search(lists, cc, x, k, nprobe)
            _same(D, I, Dr, Ir, "nlist %d k %d nprobe %d" % (nlist, k, nprobe))
    finally:
        g.close()


def test_more_queries_than_workgroups():
    """nq > 65535: both kernels walk their queries grid-stride"""
    nbits, nlist = 64, 16
    base = BR.clustered_codes(3000, nbits, 8, seed=41, dup_frac=0.2)
    cc = base[:nlist].copy()
    lists = BR.assign_lists(base, cc)
    g = _index(nbits, nlist, base, cc)
    try:
        x = _queries(base, 70000, nbits, 43)
        D, I = g.binivf_search(x, 5, _args(4, 0, 1e4))
        rows = np.concatenate([np.arange(0, 300), np.arange(65400, 70000, 7)])
        Dr, Ir = BR.search(lists, cc, x, 5, 4, 0, 1e4, rows=rows)
        _same(D[rows], I[rows], Dr, Ir, "nq 70000")
        Dc, Ic = g.binivf_assign(x, 3)
        Dcr, Icr = BR.coarse(x[rows], cc, 3)
        assert np.array_equal(Ic[rows], Icr) and np.array_equal(Dc[rows], Dcr)
    finally:
        g.close()


def test_search_large_batches_and_device_entry():
    nbits, nlist = 256, 64
    base = BR.clustered_codes(30000, nbits, 48, flip=0.04, seed=3, dup_frac=0.1)
    cc = BR.train(base[:nlist * 50], nlist)
    lists = BR.assign_lists(base, cc)
    g = _index(nbits, nlist, base, cc)
    try:
        x = _queries(base, 16384, nbits, 11)
        D, I = g.binivf_search(x, 10, _args(20))
        Dr, Ir = BR.search(lists, cc, x, 10, 20)
        _same(D, I, Dr, Ir, "nq 16384")
        D1, I1 = g.binivf_search(x[:1000], 100, _args(nlist))
        Dr1, Ir1 = BR.search(lists, cc, x[:1000], 100, nlist)
        _same(D1, I1, Dr1, Ir1, "nq 1000")
        # the device entry returns what the host entry returns
        dx = torch.from_numpy(x).cuda()
        dD = torch.empty((x.shape[0], 10), dtype=torch.float32, device="cuda")
        dI = torch.empty((x.shape[0], 10), dtype=torch.int64, device="cuda")
        g.binivf_search_device(dx.data_ptr(), x.shape[0], 10, _args(20), dD.data_ptr(), dI.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(dI.cpu().numpy(), I) and np.array_equal(dD.cpu().numpy(), D)
        assert g.binivf_stats() == (0, 0)   # the counters run only while profiling
        g.profile_enable(1)
        g.binivf_search_device(dx.data_ptr(), x.shape[0], 10, _args(20), dD.data_ptr(), dI.data_ptr())
        torch.cuda.synchronize()
        q, adm = g.binivf_stats(reset=True)
        g.profile_enable(0)
        assert q == x.shape[0] and adm > 0
        assert np.array_equal(dI.cpu().numpy(), I) and np.array_equal(dD.cpu().numpy(), D)
    finally:
        g.close()


def test_filters_and_score_windows():
    nbits, nlist = 128, 16
    n = 8000
    base = BR.clustered_codes(n, nbits, 12, flip=0.03, seed=21, dup_frac=0.2)
    cc = BR.train(base[:nlist * 60], nlist)
    lists = BR.assign_lists(base, cc)
    g = api.GammaHip(0)
    try:
        g.binivf_init(nbits, nlist)
        g.binivf_set_trained(cc)
        vid2doc = np.arange(n) // 2   # two vectors per document
        g.vid2docid_append(vid2doc.astype(np.int32))
        g.binivf_add(base, 0)
        rng = np.random.default_rng(5)
        deleted = rng.choice(n // 2, 300, replace=False)
        g.bitmap_upload(np.zeros(n // 16 + 1, np.uint8), n // 2)
        g.bitmap_set(deleted)
        g.delete(np.concatenate([2 * deleted, 2 * deleted + 1]))   # Delete only counts
        live = np.nonzero(~np.isin(np.arange(n) // 2, deleted))[0]
        x = base[rng.choice(live, 40)].copy()   # copies of live base rows: distance 0 under a widened window
        r1 = rng.choice(n // 2, 2500, replace=False)
        r2 = np.arange(1000, 2000)
        for ranges in (None, [(r1, False)], [(r2, True)], [(r1, False), (r2, True)], [([], False)]):
            f = BR.Filter(deleted=deleted, ranges=ranges, vid2doc=vid2doc)
            rf = None if ranges is None else [api.make_range_filter(d, b_not_in=b) for d, b in ranges]
            for lo, hi in ((None, None), (0, 1e4), (4, 12), (0, 0)):
                for k, nprobe in ((10, 4), (100, 16), (7, 40)):
                    D, I = g.binivf_search(x, k, _args(nprobe, lo, hi, range_filters=rf))
                    Dr, Ir = BR.search(lists, cc, x, k, nprobe, lo, hi, filt=f)
                    _same(D, I, Dr, Ir, "ranges %s window %s %s k %d" % (ranges is not None, lo, hi, k))
        # the default window excludes an exact duplicate (Hamming 0), [0, 1e4] keeps it
        D, I = g.binivf_search(x, 5, _args(nlist))
        assert (D > 0).all()
        D, I = g.binivf_search(x, 5, _args(nlist, 0, 1e4))
        assert (D[:, 0] == 0).all()
        # empty slots: a window nothing passes
        D, I = g.binivf_search(x, 5, _args(nlist, 1e5, 2e5))
        assert (I == -1).all() and (D == np.float32(2147483648.0)).all()
    finally:
        g.close()


def test_realtime_adds_with_searches_between():
    nbits, nlist = 96, 16
    allc = BR.clustered_codes(9000, nbits, 10, flip=0.05, seed=31, dup_frac=0.1)
    cc = BR.train(allc[:nlist * 40], nlist)
    g = api.GammaHip(0)
    try:
        g.binivf_init(nbits, nlist, bucket_init_size=50)   # small buckets: the lists grow while searched
        g.binivf_set_trained(cc)
        lists = None
        x = _queries(allc, 50, nbits, 3)
        first = 0
        for step, m in enumerate((1, 7, 500, 2000, 6492)):
            batch = allc[first:first + m]
            g.binivf_add(batch, first)
            lists = BR.assign_lists(batch, cc, first, lists)
            first += m
            for l in range(nlist):
                ids, codes = g.get_list(l)
                assert np.array_equal(ids, lists[l][0]) and np.array_equal(codes, lists[l][1])
            D, I = g.binivf_search(x, 20, _args(6, 0, 1e4))
            Dr, Ir = BR.search(lists, cc, x, 20, 6, 0, 1e4)
            _same(D, I, Dr, Ir, "step %d" % step)
    finally:
        g.close()


def test_entry_points_and_limits():
    nbits, nlist = 64, 8
    base = BR.clustered_codes(500, nbits, 4, seed=1)
    g = api.GammaHip(0)
    try:
        g.binivf_init(nbits, nlist)
        with pytest.raises(api.GammaHipError):   # Add before training
            g.binivf_add(base, 0)
        g.binivf_set_trained(base[:nlist])
        g.binivf_add(base, 0)
        with pytest.raises(api.GammaHipError):   # the float models' entries refuse a binary handle
            g.ivfflat_search(np.zeros((1, nbits), np.float32), 1, _args(1))
        with pytest.raises(api.GammaHipError):
            g.ivfpq_search(np.zeros((1, nbits), np.float32), 1, _args(1))
        with pytest.raises(api.GammaHipError) as e:   # k beyond the LDS heap
            g.binivf_search(base[:2], 4097, _args(1))
        assert "4096" in str(e.value)
        D, I = g.binivf_search(base[:3], 4096, _args(nlist))   # the largest k, heap replay beyond the all-lane sifts
        Dr, Ir = BR.search(BR.assign_lists(base, base[:nlist]), base[:nlist], base[:3], 4096, nlist)
        _same(D, I, Dr, Ir, "k 4096")
    finally:
        g.close()
    with pytest.raises(api.GammaHipError):
        g2 = api.GammaHip(0)
        try:
            g2.binivf_init(60, 4)   # nbits % 8 != 0
        finally:
            g2.close()
