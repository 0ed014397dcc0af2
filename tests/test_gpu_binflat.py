"""GPU: exact Hamming (binary flat) search through the C ABI (gamma_hip_binflat_*) against the one-list yardstick
(tests/binflat_ref.py = tests/binivf_ref.py::search over ONE list holding every code in vid order, nprobe 1): labels equal
and distance BYTES equal at every rank -- with integer distances nearly every query has a tie at the cut, so the order
inside ties is what these tests are about.  Sizes are written in the kernels' row chunk C."""
import numpy as np
import pytest
import torch

from gamma_amd import _lib, api
from gamma_amd._lib import GammaHipError
from tests import binflat_ref as BF
from tests import binivf_ref as BR

pytestmark = pytest.mark.gpu

NQ = 130
NBITS = (8, 40, 64, 128, 256, 2048)   # bytes, dwords and 16-byte loads of the rows
_cache = {}


def _chunk():
    return int(_lib.load().gamma_hip_binflat_chunk_rows())


def _data(nbits):
    """(base [2C + 37], queries [NQ], their distance matrix), once per nbits"""
    if nbits not in _cache:
        C = _chunk()
        base = BR.clustered_codes(2 * C + 37, nbits, 24, flip=0.04, seed=nbits, dup_frac=0.1)
        rng = np.random.default_rng(nbits + 1)
        new = BR.clustered_codes(NQ - NQ // 2, nbits, 16, flip=0.08, seed=nbits + 2, dup_frac=0.0)
        x = np.ascontiguousarray(np.concatenate([base[rng.integers(0, base.shape[0], NQ // 2)], new]))
        _cache[nbits] = (base, x, BF.hamming_matrix(x, base))
    return _cache[nbits]


def _rows(name, C):
    return {"0": 0, "1": 1, "9": 9, "99": 99, "999": 999, "C-1": C - 1, "C": C, "C+1": C + 1, "2C+37": 2 * C + 37}[name]


def _args(lo=None, hi=None, **kw):
    return api.SearchArgs(nprobe=1, min_score=lo, max_score=hi, **kw)


def _same(D, I, Dr, Ir, what=""):
    assert I.shape == Ir.shape and D.dtype == np.float32
    assert np.array_equal(I, Ir) and D.tobytes() == Dr.tobytes(), what


def _store(nbits, codes):
    g = api.GammaHip(0)
    g.binflat_init(nbits)
    g.binflat_append(codes)
    return g


# k - 1 for k = 1, 10, 100, 1000 is 0, 9, 99, 999
@pytest.mark.parametrize("rows", ["0", "1", "9", "99", "999", "C-1", "C", "C+1", "2C+37"])
@pytest.mark.parametrize("nbits", NBITS)
def test_grid(nbits, rows):
    C = _chunk()
    N = _rows(rows, C)
    base, x, dm = _data(nbits)
    g = _store(nbits, base[:N])
    try:
        assert g.binflat_count() == N
        for k in (1, 10, 100, 1000):   # k > N in the small stores
            Dr, Ir = BF.search(dm[:, :N], k, 0, 1e4)
            for nq in (1, 7, 33, NQ):
                D, I = g.binflat_search(x[:nq], k, _args(0, 1e4))
                _same(D, I, Dr[:nq], Ir[:nq], "nbits %d N %d k %d nq %d" % (nbits, N, k, nq))
        Dr, Ir = BF.search(dm[:, :N], 10)   # the default window
        D, I = g.binflat_search(x, 10, _args())
        _same(D, I, Dr, Ir, "default window")
    finally:
        g.close()


def test_k_4096():
    C = _chunk()
    base, x, dm = _data(64)
    g = _store(64, base[:C + 1])
    try:
        D, I = g.binflat_search(x[:3], 4096, _args(0, 1e4))
        _same(D, I, *BF.search(dm[:3, :C + 1], 4096, 0, 1e4))
        with pytest.raises(GammaHipError):
            g.binflat_search(x[:3], 4097, _args(0, 1e4))
    finally:
        g.close()


def test_tie_heavy():
    """nine distinct distances over 3000 rows: every rank is inside a tie"""
    rng = np.random.default_rng(8)
    base = rng.integers(0, 256, (3000, 1), dtype=np.uint8)
    x = rng.integers(0, 256, (33, 1), dtype=np.uint8)
    dm = BF.hamming_matrix(x, base)
    g = _store(8, base)
    try:
        for k in (1, 10, 100, 1000):
            for lo, hi in ((0, 1e4), (None, None), (2, 5)):
                D, I = g.binflat_search(x, k, _args(lo, hi))
                _same(D, I, *BF.search(dm, k, lo, hi), "k %d window %s %s" % (k, lo, hi))
    finally:
        g.close()


def test_far_to_near_rows_run_in_sub_batches():
    """rows sorted by decreasing distance to the query: nearly every row is a candidate; with a small workspace budget the
    queries run in several sub-batches and the answer stays exact"""
    C = _chunk()
    base, _, _ = _data(256)
    rng = np.random.default_rng(12)
    q = base[17].copy()
    order = np.argsort(-BR.hamming(q, base), kind="stable")
    rows = np.ascontiguousarray(base[order])
    x = np.repeat(q[None, :], 5, axis=0)
    for i in range(1, 5):   # the query and four codes a few bits from it
        x[i, rng.integers(0, x.shape[1], 3)] ^= np.uint8(1 << i)
    dm = BF.hamming_matrix(x, rows)
    g = _store(256, rows)
    try:
        g.set_dist_budget(64 * 1024)
        g.binflat_stats(reset=True)
        for k in (10, 100):
            D, I = g.binflat_search(x, k, _args(0, 1e4))
            _same(D, I, *BF.search(dm, k, 0, 1e4), "k %d" % k)
        queries, cand, adm, sub = g.binflat_stats()
        assert queries == 10 and sub > 2
        assert cand == BF.design_candidates(dm, 10, C, 0, 1e4) + BF.design_candidates(dm, 100, C, 0, 1e4)
        assert cand > 10 * rows.shape[0] // 2
    finally:
        g.close()


def test_windows_and_padding():
    base, x, dm = _data(128)
    N = 5000
    g = _store(128, base[:N])
    try:
        xd = base[:30]   # exact duplicates of stored rows
        D, _ = g.binflat_search(xd, 3, _args())
        assert (D > 0).all()   # the default window [FLT_MIN, FLT_MAX] excludes distance 0
        D, I = g.binflat_search(xd, 3, _args(0, 1e4))
        assert (D[:, 0] == 0).all()
        _same(D, I, *BF.search(BF.hamming_matrix(xd, base[:N]), 3, 0, 1e4))
        for lo, hi in ((4, 12), (0, 0), (30, 40)):
            D, I = g.binflat_search(x, 20, _args(lo, hi))
            _same(D, I, *BF.search(dm[:, :N], 20, lo, hi), "window %s %s" % (lo, hi))
        D, I = g.binflat_search(x, 5, _args(1e5, 2e5))   # a window nothing passes
        assert (I == -1).all() and D.tobytes() == np.full(D.shape, 2147483648.0, np.float32).tobytes()
    finally:
        g.close()


@pytest.mark.parametrize("multi", [False, True])
def test_filters(multi):
    """delete bitmap + a range result + a NOT range, on vids and (multi) on two-vector documents"""
    C = _chunk()
    base, x, dm = _data(128)
    n = C + 900
    g = _store(128, base[:n])
    try:
        ndoc = n // 2 if multi else n
        vid2doc = np.arange(n) // 2 if multi else None
        if multi:
            g.vid2docid_append(vid2doc.astype(np.int32))
        rng = np.random.default_rng(5)
        deleted = rng.choice(ndoc, 300, replace=False)
        g.bitmap_upload(np.zeros(ndoc // 8 + 1, np.uint8), ndoc)
        g.bitmap_set(deleted)
        r1 = rng.choice(ndoc, ndoc // 3, replace=False)
        r2 = np.arange(400, 1500)
        for ranges in (None, [(r1, False)], [(r2, True)], [(r1, False), (r2, True)], [([], False)]):
            f = BR.Filter(deleted=deleted, ranges=ranges, vid2doc=vid2doc)
            rf = None if ranges is None else [api.make_range_filter(d, b_not_in=b) for d, b in ranges]
            for lo, hi in ((None, None), (0, 1e4)):
                for k in (10, 100):
                    D, I = g.binflat_search(x[:40], k, _args(lo, hi, range_filters=rf))
                    _same(D, I, *BF.search(dm[:40, :n], k, lo, hi, filt=f), "ranges %s k %d" % (ranges is not None, k))
    finally:
        g.close()


def test_device_column_filter():
    base, x, dm = _data(64)
    n = 3000
    g = _store(64, base[:n])
    try:
        col = np.random.default_rng(3).integers(0, 100, n).astype(np.int32)
        g.field_append(1, col)
        D, I = g.binflat_search(x[:20], 10, _args(0, 1e4, field_filters=[(1, 20, 60, True, False)]))
        f = BR.Filter(ranges=[(np.nonzero((col >= 20) & (col < 60))[0], False)])
        _same(D, I, *BF.search(dm[:20, :n], 10, 0, 1e4, filt=f))
    finally:
        g.close()


def test_append_in_pieces_across_growth():
    C = _chunk()
    base, x, dm = _data(256)
    g = api.GammaHip(0)
    try:
        g.binflat_init(256)
        mem0 = g.total_mem_bytes()
        n = 0
        for piece in (700, 900, C, 1, 2000):   # the array grows between the searches
            g.binflat_append(base[n:n + piece])
            n += piece
            assert g.binflat_count() == n
            D, I = g.binflat_search(x[:33], 10, _args(0, 1e4))
            _same(D, I, *BF.search(dm[:33, :n], 10, 0, 1e4), "after %d rows" % n)
        assert g.total_mem_bytes() - mem0 >= n * 32
    finally:
        g.close()


def test_device_entry():
    C = _chunk()
    base, x, dm = _data(256)
    N = C + 1
    g = _store(256, base[:N])
    try:
        D, I = g.binflat_search(x, 10, _args(0, 1e4))
        dx = torch.from_numpy(x).cuda()
        dD = torch.empty((NQ, 10), dtype=torch.float32, device="cuda")
        dI = torch.empty((NQ, 10), dtype=torch.int64, device="cuda")
        g.binflat_search_device(dx.data_ptr(), NQ, 10, _args(0, 1e4), dD.data_ptr(), dI.data_ptr())
        g.synchronize()
        _same(dD.cpu().numpy(), dI.cpu().numpy(), D, I)
        _same(D, I, *BF.search(dm[:, :N], 10, 0, 1e4))
    finally:
        g.close()


def test_init_rules():
    g = api.GammaHip(0)
    try:
        g.ivfflat_init(16, 4)
        with pytest.raises(GammaHipError):   # a float model's handle
            g.binflat_init(128)
    finally:
        g.close()
    g = api.GammaHip(0)
    try:
        g.raw_init(16)
        with pytest.raises(GammaHipError):
            g.binflat_init(128)
    finally:
        g.close()
    g = api.GammaHip(0)
    try:
        assert g.binflat_count() == -1
        with pytest.raises(GammaHipError):
            g.binflat_init(12)
        with pytest.raises(GammaHipError):
            g.binflat_init(4096)
        g.binflat_init(64)
        g.binflat_init(64)
        with pytest.raises(GammaHipError):   # another nbits
            g.binflat_init(128)
        with pytest.raises(GammaHipError):
            g.binivf_init(128, 4)
        g.binivf_init(64, 4)   # flat first, then the IVF model
    finally:
        g.close()
    g = api.GammaHip(0)
    try:
        with pytest.raises(GammaHipError):
            g.binflat_append(np.zeros((1, 8), np.uint8))
        g.binivf_init(64, 4)
        with pytest.raises(GammaHipError):
            g.binflat_init(128)
        g.binflat_init(64)     # the IVF model first, then flat
    finally:
        g.close()


def test_binivf_search_unchanged_beside_the_flat_store():
    nbits, nlist = 128, 16
    base, x, dm = _data(nbits)
    n = 6000
    cc = BR.train(base[:nlist * 60], nlist)
    lists = BR.assign_lists(base[:n], cc)
    g = api.GammaHip(0)
    try:
        g.binivf_init(nbits, nlist)
        g.binivf_set_trained(cc)
        g.binivf_add(base[:n], 0)
        before = g.binivf_search(x, 10, api.SearchArgs(nprobe=8, min_score=0, max_score=1e4))
        g.binflat_init(nbits)
        g.binflat_append(base[:n])
        D, I = g.binflat_search(x, 10, _args(0, 1e4))
        _same(D, I, *BF.search(dm[:, :n], 10, 0, 1e4))
        after = g.binivf_search(x, 10, api.SearchArgs(nprobe=8, min_score=0, max_score=1e4))
        _same(after[0], after[1], before[0], before[1])
        _same(after[0], after[1], *BR.search(lists, cc, x, 10, 8, 0, 1e4))
    finally:
        g.close()


def test_stats():
    """random order: the candidates are chunk 0 plus a few rows per later chunk; admissions are the serial heap's"""
    C = _chunk()
    N = 2 * C + 37
    rng = np.random.default_rng(77)
    base = rng.integers(0, 256, (N, 32), dtype=np.uint8)
    x = rng.integers(0, 256, (7, 32), dtype=np.uint8)
    dm = BF.hamming_matrix(x, base)
    g = _store(256, base)
    try:
        g.binflat_stats(reset=True)
        D, I = g.binflat_search(x, 10, _args(0, 1e4))
        _same(D, I, *BF.search(dm, 10, 0, 1e4))
        queries, cand, adm, sub = g.binflat_stats(reset=True)
        assert queries == 7 and sub == 1
        assert adm == BF.admissions(dm, 10, 0, 1e4)
        assert adm <= cand <= 7 * (C + N // 8)
        assert cand == BF.design_candidates(dm, 10, C, 0, 1e4)
        assert g.binflat_stats() == (0, 0, 0, 0)
    finally:
        g.close()
