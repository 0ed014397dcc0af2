"""GPU: the binary IVF scan of large batches list-major (gamma_hip_binivf_set_lm_scan, binivf_lm.hip) against the model's
restatement (tests/binivf_ref.py), strictly: labels and distance bits at every rank.  Every case sets the switch with
min_nq 1 under scan mode 0 (the automatic mode spreads small calls before the switch is asked) and checks through binivf_lm_stats that the list-major chain answered every query and k_bin_scan none.  A yardstick
answer is computed once for the largest query set and sliced: the queries of a call are independent."""
import numpy as np
import pytest
import torch

from gamma_amd import api
from tests import binivf_ref as BR

pytestmark = pytest.mark.gpu

C, QT, AUTO_MIN_NQ = api.binivf_lm_shape()
NQS = (1, QT - 1, QT, QT + 1, 2 * QT + 3)
BIG = 8 << 30


def _args(nprobe, lo=0, hi=1e4, **kw):
    return api.SearchArgs(nprobe=nprobe, min_score=lo, max_score=hi, **kw)


def _same(D, I, Dr, Ir, what=""):
    assert I.shape == Ir.shape
    bad = np.nonzero((I != Ir).any(axis=1) | (D.view(np.uint32) != Dr.view(np.uint32)).any(axis=1))[0]
    assert bad.size == 0, "%s: %d rows differ, first %d: dev %s %s ref %s %s" % (
        what, bad.size, bad[0], D[bad[0]][:8], I[bad[0]][:8], Dr[bad[0]][:8], Ir[bad[0]][:8])


def _on(g):
    g.binivf_set_scan_mode(0)
    g.binivf_set_lm_scan(1, min_nq=1)


def _filled(nbits, cc, lists, bucket_init=1000):
    """a handle whose list l holds exactly lists[l] = (vids, codes), the list-major switch on for every call"""
    g = api.GammaHip(0)
    g.binivf_init(nbits, cc.shape[0], bucket_init_size=bucket_init)
    g.binivf_set_trained(cc)
    for l, (v, c) in enumerate(lists):
        if v.size:
            g.add_keys(l, v, c)
    _on(g)
    return g


def _split(codes, lens, seed=0):
    vids = np.random.default_rng(seed).permutation(int(sum(lens))).astype(np.int64)
    at = np.concatenate([[0], np.cumsum(lens)])
    return [(vids[a:b], np.ascontiguousarray(codes[a:b])) for a, b in zip(at[:-1], at[1:])]


def _lm(g, fn):
    """binivf_lm_stats and binivf_stats of the searches fn makes"""
    g.profile_enable(1)
    g.binivf_lm_stats(reset=True)
    g.binivf_stats(reset=True)
    fn()
    st = g.binivf_lm_stats(reset=True), g.binivf_stats(reset=True)
    g.profile_enable(0)
    return st


def _check(g, x, k, args, Dr, Ir, what):
    """one search of x against the yardstick's rows; the list-major chain answered all of it"""
    nq = x.shape[0]
    st, bst = _lm(g, lambda: _same(*g.binivf_search(x, k, args), Dr[:nq], Ir[:nq], "%s nq %d k %d" % (what, nq, k)))
    assert st[0] == nq and st[4] == 0 and bst[0] == nq, (what, nq, st, bst)
    return st


@pytest.fixture(scope="module")
def edges():
    """nlist 8, lists of 0, 1, C - 1, C, C + 1 and 3C + 5 rows (and two ordinary ones), 256 bits: 16-byte loads"""
    nbits = 256
    lens = [0, 1, C - 1, C, C + 1, 3 * C + 5, 300, 77]
    codes = BR.clustered_codes(sum(lens), nbits, 12, flip=0.05, seed=1, dup_frac=0.1)
    lists = _split(codes, lens)
    cc = np.ascontiguousarray(np.stack([l[1][0] if l[0].size else codes[-1] ^ np.uint8(0x55) for l in lists]))
    rng = np.random.default_rng(2)
    x = np.ascontiguousarray(np.concatenate([codes[rng.integers(0, codes.shape[0], NQS[-1] - 9)],
                                             BR.clustered_codes(9, nbits, 12, flip=0.08, seed=3, dup_frac=0.0)]))
    g = _filled(nbits, cc, lists)
    yield g, lists, cc, x
    g.close()


@pytest.mark.parametrize("k", [1, 10, 16, 100, 300])
def test_tiles_and_chunk_edges(edges, k):
    """1, QT - 1, QT, QT + 1 and 2 QT + 3 queries on every list (nprobe 8 of 8), ragged tiles (nprobe 1, 3), -1 probe
    slots (the request's nprobe 0 is the model's 20 > nlist)"""
    g, lists, cc, x = edges
    for nprobe in (8, 1, 3, 0):
        Dr, Ir = BR.search(lists, cc, x, k, nprobe, 0, 1e4)
        for nq in (NQS if nprobe == 8 else NQS[3:]):
            _check(g, x[:nq], k, _args(nprobe), Dr, Ir, "edges nprobe %d" % nprobe)
    Dr, Ir = BR.search(lists, cc, x[:QT + 1], k, 8)
    _check(g, x[:QT + 1], k, _args(8, None, None), Dr, Ir, "edges, default window")   # (it excludes distance 0)


def test_k_4096(edges):
    g, lists, cc, x = edges
    xs = x[:QT + 1]
    Dr, Ir = BR.search(lists, cc, xs, 4096, 2, 0, 1e4)
    assert (Ir == -1).any()   # more slots than valid rows probed
    _check(g, xs, 4096, _args(2), Dr, Ir, "k 4096")


@pytest.mark.parametrize("nbits", [96, 72, 2048])
def test_load_widths(nbits):
    """dword and byte code loads; 2048 bits: one row per thread in four passes, histograms in sub-tiles of the tile"""
    nlist = 8
    base = BR.clustered_codes(3000, nbits, 10, flip=0.04, seed=nbits, dup_frac=0.1)
    cc = base[np.random.default_rng(nbits).choice(3000, nlist, replace=False)].copy()
    lists = BR.assign_lists(base, cc)
    g = _filled(nbits, cc, lists)
    try:
        x = np.ascontiguousarray(np.concatenate([base[::3000 // QT][:QT], BR.clustered_codes(3, nbits, 10, flip=0.08, seed=5)]))
        for k, nprobe in ((10, 3), (100, 8)):
            _check(g, x, k, _args(nprobe), *BR.search(lists, cc, x, k, nprobe, 0, 1e4), "nbits %d" % nbits)
    finally:
        g.close()


def test_row_orders():
    """strictly falling rows: every row of every chunk is a candidate; all-equal rows: every cut is a tie"""
    nbits = 2048
    rng = np.random.default_rng(8)
    q = rng.integers(0, 256, (1, nbits // 8), dtype=np.uint8)
    m = min(nbits, 2 * C - 3)   # more rows than a chunk, distances m, m - 1, .., 1
    bits = np.unpackbits(np.repeat(q, m, axis=0), axis=1, bitorder="little")
    for i in range(m):
        bits[i, :m - i] ^= 1
    falling = np.packbits(bits, axis=1, bitorder="little")
    equal = np.repeat(falling[m // 2:m // 2 + 1], m, axis=0)
    lists = _split(np.concatenate([falling, equal]), [m, m], seed=3)
    cc = np.ascontiguousarray(np.stack([falling[-1], equal[0]]))   # list 0 is the query's first probe (distance 1)
    g = _filled(nbits, cc, lists, bucket_init=m)
    try:
        x = np.repeat(q, 3, axis=0)
        for k in (1, 10, 100):
            st = _check(g, x, k, _args(1), *BR.search(lists, cc, x, k, 1, 0, 1e4), "falling")
            assert st[2:4] == (3 * ((m + C - 1) // C), 3 * m), st   # candidates == the rows probed
            _check(g, x, k, _args(2), *BR.search(lists, cc, x, k, 2, 0, 1e4), "falling + equal")
    finally:
        g.close()


def test_filters_and_score_windows():
    nbits, nlist, n = 128, 16, 4000
    base = BR.clustered_codes(n, nbits, 12, flip=0.03, seed=21, dup_frac=0.2)
    cc = BR.train(base[:nlist * 60], nlist)
    lists = BR.assign_lists(base, cc)
    g = api.GammaHip(0)
    try:
        g.binivf_init(nbits, nlist)
        g.binivf_set_trained(cc)
        _on(g)
        vid2doc = np.arange(n) // 2   # two vectors per document
        g.vid2docid_append(vid2doc.astype(np.int32))
        g.binivf_add(base, 0)
        rng = np.random.default_rng(5)
        deleted = rng.choice(n // 2, 150, replace=False)
        g.bitmap_upload(np.zeros(n // 16 + 1, np.uint8), n // 2)
        g.bitmap_set(deleted)
        live = np.nonzero(~np.isin(np.arange(n) // 2, deleted))[0]
        x = base[rng.choice(live, QT + 3)].copy()   # copies of live base rows: distance 0 under a widened window
        r1 = rng.choice(n // 2, 1200, replace=False)
        r2 = np.arange(500, 1000)
        for ranges in (None, [(r1, False), (r2, True)]):
            f = BR.Filter(deleted=deleted, ranges=ranges, vid2doc=vid2doc)
            rf = None if ranges is None else [api.make_range_filter(d, b_not_in=b) for d, b in ranges]
            for lo, hi in ((None, None), (0, 1e4), (4, 12)):
                Dr, Ir = BR.search(lists, cc, x, 10, 4, lo, hi, filt=f)
                _check(g, x, 10, _args(4, lo, hi, range_filters=rf), Dr, Ir, "ranges %s window %s %s" % (ranges is not None, lo, hi))
    finally:
        g.close()


def test_sub_batches_and_fallback(edges):
    """the candidate slab alone is nprobe x the longest list x 8 bytes per query: half a budget of 5 QT slabs holds fewer
    than 3 QT queries (at least two sub-batches) and more than one tile; half a budget of one slab holds no tile"""
    g, lists, cc, x = edges
    xs = np.ascontiguousarray(np.resize(x, (3 * QT, x.shape[1])))
    ref = tuple(np.resize(a, (3 * QT, 10)) for a in BR.search(lists, cc, x, 10, 8, 0, 1e4))
    slab = 8 * g.max_list_len() * 8
    try:
        g.set_dist_budget(5 * QT * slab)
        whole = _check(g, xs, 10, _args(8), *ref, "sub-batches")
        g.set_dist_budget(slab)
        st, bst = _lm(g, lambda: _same(*g.binivf_search(xs, 10, _args(8)), *ref, "no tile fits"))
        assert st == (0, 0, 0, 0, 3 * QT) and bst[0] == 3 * QT, (st, bst)
    finally:
        g.set_dist_budget(BIG)
    assert _check(g, xs, 10, _args(8), *ref, "budget restored")[2:4] == whole[2:4]


@pytest.mark.parametrize("k,nprobe", [(1, 8), (10, 3), (100, 8)])
def test_the_spread_chain_s_candidates(edges, k, nprobe):
    """chunks, candidates and heap admissions of a call equal the spread chain's (scan mode 1, the switch off)"""
    g, lists, cc, x = edges
    xs = x[:QT + 1]
    st, bst = _lm(g, lambda: g.binivf_search(xs, k, _args(nprobe)))
    try:
        g.binivf_set_lm_scan(0)
        g.binivf_set_scan_mode(1)
        g.profile_enable(1)
        g.binivf_scan_stats(reset=True)
        g.binivf_search(xs, k, _args(nprobe))
        sp, bsp = g.binivf_scan_stats(reset=True), g.binivf_stats(reset=True)
    finally:
        g.profile_enable(0)
        _on(g)
    assert (st[0], st[2], st[3]) == sp[:3] and st[1] > 0 and bst == bsp, (st, sp, bst, bsp)


def test_device_entry_and_realtime_add():
    nbits, nlist = 96, 16
    allc = BR.clustered_codes(5000, nbits, 10, flip=0.05, seed=31, dup_frac=0.1)
    cc = BR.train(allc[:nlist * 40], nlist)
    g = api.GammaHip(0)
    try:
        g.binivf_init(nbits, nlist, bucket_init_size=50)   # small buckets: the lists grow between the searches
        g.binivf_set_trained(cc)
        _on(g)
        x = np.ascontiguousarray(allc[::5000 // (QT + 5)])
        nq, k = x.shape[0], 20
        dx = torch.from_numpy(x).cuda()
        dD = torch.empty((nq, k), dtype=torch.float32, device="cuda")
        dI = torch.empty((nq, k), dtype=torch.int64, device="cuda")
        lists, first = None, 0
        for m in (1500, 3500):   # the second search reads the version the second add published
            g.binivf_add(allc[first:first + m], first)
            lists = BR.assign_lists(allc[first:first + m], cc, first, lists)
            first += m
            st, _ = _lm(g, lambda: (g.binivf_search_device(dx.data_ptr(), nq, k, _args(6), dD.data_ptr(), dI.data_ptr()),
                                    torch.cuda.synchronize()))
            assert st[0] == nq and st[4] == 0
            _same(dD.cpu().numpy(), dI.cpu().numpy(), *BR.search(lists, cc, x, k, 6, 0, 1e4), "device entry after %d rows" % first)
    finally:
        g.close()


def test_switch_off_by_default(edges):
    g, lists, cc, x = edges
    assert C > 0 and QT > 0 and AUTO_MIN_NQ > 0
    auto_max_nq = api.binivf_scan_shape()[1]
    n = auto_max_nq + 1
    xs = np.ascontiguousarray(np.resize(x[:7], (n, x.shape[1])))
    ref = tuple(np.resize(a, (n, 10)) for a in BR.search(lists, cc, x[:7], 10, 3, 0, 1e4))
    fresh = api.GammaHip(0)
    try:
        fresh.binivf_init(64, 4)
        assert fresh.binivf_lm_scan() == (0, 0)   # the default
    finally:
        fresh.close()
    try:
        g.binivf_set_scan_mode(-1)
        g.binivf_set_lm_scan(0)
        st, bst = _lm(g, lambda: _same(*g.binivf_search(xs, 10, _args(3)), *ref, "switch off"))
        assert st == (0, 0, 0, 0, 0) and bst[0] == n
        g.binivf_set_lm_scan(1, min_nq=n + 1)   # on, but the call is below min_nq
        assert g.binivf_lm_scan() == (1, n + 1)
        assert _lm(g, lambda: g.binivf_search(xs, 10, _args(3)))[0] == (0, 0, 0, 0, 0)
        with pytest.raises(api.GammaHipError):
            g.binivf_set_lm_scan(1, min_nq=-1)
    finally:
        _on(g)
    fl = api.GammaHip(0)   # a float model's handle
    try:
        fl.raw_init(16)
        fl.ivfflat_init(16, 4)
        for call in (lambda: fl.binivf_set_lm_scan(1), fl.binivf_lm_scan, fl.binivf_lm_stats):
            with pytest.raises(api.GammaHipError):
                call()
    finally:
        fl.close()
