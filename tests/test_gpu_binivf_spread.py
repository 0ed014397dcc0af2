"""GPU: the binary IVF scan of one query spread over the device (gamma_hip_binivf_set_scan_mode 1, binivf_spread.hip) against
the model's restatement (tests/binivf_ref.py), strictly: labels and distance bits at every rank, under mode 1 and again under
mode 0 (one wave per query).  Lists are filled directly with add_keys, so their lengths are chosen around the chunk size."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gamma_amd import api
from tests import binivf_ref as BR
from tests import binivf_spread_ref as SR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, AUTO_MAX_NQ = api.binivf_scan_shape()
BIG = 8 << 30


def _args(nprobe, lo=None, hi=None, **kw):
    return api.SearchArgs(nprobe=nprobe, min_score=lo, max_score=hi, **kw)


def _same(D, I, Dr, Ir, what=""):
    assert I.shape == Ir.shape
    bad = np.nonzero((I != Ir).any(axis=1) | (D.view(np.uint32) != Dr.view(np.uint32)).any(axis=1))[0]
    assert bad.size == 0, "%s: %d rows differ, first %d: dev %s %s ref %s %s" % (
        what, bad.size, bad[0], D[bad[0]][:8], I[bad[0]][:8], Dr[bad[0]][:8], Ir[bad[0]][:8])


def _filled(nbits, cc, lists, bucket_init=1000):
    """a handle whose list l holds exactly lists[l] = (vids, codes)"""
    g = api.GammaHip(0)
    g.binivf_init(nbits, cc.shape[0], bucket_init_size=bucket_init)
    g.binivf_set_trained(cc)
    for l, (v, c) in enumerate(lists):
        if v.size:
            g.add_keys(l, v, c)
    return g


def _split(codes, lens, seed=0):
    """consecutive runs of codes as lists of the given lengths, with vids that are a permutation"""
    vids = np.random.default_rng(seed).permutation(int(sum(lens))).astype(np.int64)
    out, at = [], 0
    for m in lens:
        out.append((vids[at:at + m], np.ascontiguousarray(codes[at:at + m])))
        at += m
    return out


def _both_modes(g, lists, cc, x, k, nprobe, lo=None, hi=None, filt=None, what="", ref=None, **kw):
    """the search under mode 1 and under mode 0 against the yardstick; returns the yardstick's answer"""
    Dr, Ir = ref if ref is not None else BR.search(lists, cc, x, k, nprobe, lo, hi, filt=filt)
    for mode in (1, 0):
        g.binivf_set_scan_mode(mode)
        D, I = g.binivf_search(x, k, _args(nprobe, lo, hi, **kw))
        _same(D, I, Dr, Ir, "%s mode %d k %d nprobe %d nq %d" % (what, mode, k, nprobe, x.shape[0]))
    return Dr, Ir


def _spread_queries(g, fn):
    """the queries the spread chain answered while fn ran, and the whole counter tuple"""
    g.profile_enable(1)
    g.binivf_scan_stats(reset=True)
    fn()
    st = g.binivf_scan_stats(reset=True)
    g.profile_enable(0)
    return st


@pytest.fixture(scope="module")
def edges():
    """nlist 8, lists of 0, 1, C - 1, C, C + 1 and 3C + 5 rows (and two ordinary ones), 256 bits"""
    nbits = 256
    lens = [0, 1, C - 1, C, C + 1, 3 * C + 5, 300, 77]
    codes = BR.clustered_codes(sum(lens), nbits, 12, flip=0.05, seed=1, dup_frac=0.1)
    lists = _split(codes, lens)
    # centroids: one row of every list (any code for the empty one), so that queries probe the lists in varied orders
    cc = np.ascontiguousarray(np.stack([l[1][0] if l[0].size else codes[-1] ^ np.uint8(0x55) for l in lists]))
    rng = np.random.default_rng(2)
    x = np.ascontiguousarray(np.concatenate([codes[rng.integers(0, codes.shape[0], 4)],
                                             BR.clustered_codes(3, nbits, 12, flip=0.08, seed=3, dup_frac=0.0)]))
    g = _filled(nbits, cc, lists)
    yield g, lists, cc, x
    g.close()


@pytest.mark.parametrize("k", [1, 10, 16, 100, 300])
def test_chunk_edges(edges, k):
    g, lists, cc, x = edges
    for nprobe in (1, 3, 8):
        for nq in (1, 7):
            _both_modes(g, lists, cc, x[:nq], k, nprobe, 0, 1e4, what="edges")
    _both_modes(g, lists, cc, x, k, 8, what="edges, default window")


def test_heap_forms_and_empty_slots(edges):
    g, lists, cc, x = edges
    _both_modes(g, lists, cc, x, 1000, 8, 0, 1e4, what="k 1000")           # the sequential heap
    Dr, Ir = _both_modes(g, lists, cc, x, 4096, 2, 0, 1e4, what="k 4096")   # more slots than valid rows probed
    assert (Ir == -1).any() and (Dr[Ir == -1] == BR.EMPTY_D).all()
    Dr, Ir = _both_modes(g, lists, cc, x, 20, 8, 1e5, 2e5, what="empty window")
    assert (Ir == -1).all()


def test_not_enough_centroids(edges):
    """the request's nprobe 0: the model's 20 > nlist 8, probe slots of -1"""
    g, lists, cc, x = edges
    for k in (10, 100):
        _both_modes(g, lists, cc, x, k, 0, 0, 1e4, what="nprobe 20 of 8")


@pytest.mark.parametrize("nbits", [32, 40, 200, 256, 2048])
def test_load_widths(nbits):
    """16-byte, dword and byte code loads; duplicates put ties at nearly every cut"""
    nlist = 8
    base = BR.clustered_codes(3000, nbits, 10, flip=0.04, seed=nbits, dup_frac=0.1)
    cc = base[np.random.default_rng(nbits).choice(3000, nlist, replace=False)].copy()
    lists = BR.assign_lists(base, cc)
    g = _filled(nbits, cc, lists)
    try:
        x = np.ascontiguousarray(np.concatenate([base[::500], BR.clustered_codes(3, nbits, 10, flip=0.08, seed=5)]))
        for k, nprobe in ((10, 3), (100, 8)):
            _both_modes(g, lists, cc, x, k, nprobe, 0, 1e4, what="nbits %d" % nbits)
    finally:
        g.close()


def test_worst_case_for_candidates():
    """a list whose rows come from far to near, every one strictly nearer than all before it: every row of every chunk is a
    candidate (the case the candidate slab is sized for); a list of equal codes: no candidate once k rows precede a chunk"""
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
        for k in (1, 10, 100):
            for nprobe in (1, 2):
                _both_modes(g, lists, cc, q, k, nprobe, 0, 1e4, what="worst case")
            g.binivf_set_scan_mode(1)
            st = _spread_queries(g, lambda: g.binivf_search(q, k, _args(1, 0, 1e4)))
            assert st == (1, (m + C - 1) // C, m, 0), (k, st)   # candidates == the valid rows probed
            assert SR.counts(lists, cc, q, k, 1, C, 0, 1e4) == (m, m, (m + C - 1) // C, m)
            st = _spread_queries(g, lambda: g.binivf_search(q, k, _args(2, 0, 1e4)))
            assert st == (1,) + SR.counts(lists, cc, q, k, 2, C, 0, 1e4)[2:0:-1] + (0,), (k, st)
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
        x = base[rng.choice(live, 12)].copy()   # copies of live base rows: distance 0 under a widened window
        r1 = rng.choice(n // 2, 2500, replace=False)
        r2 = np.arange(1000, 2000)
        for ranges in (None, [(r1, False)], [(r2, True)], [(r1, False), (r2, True)], [([], False)]):
            f = BR.Filter(deleted=deleted, ranges=ranges, vid2doc=vid2doc)
            rf = None if ranges is None else [api.make_range_filter(d, b_not_in=b) for d, b in ranges]
            for lo, hi in ((None, None), (0, 1e4), (4, 12), (0, 0)):
                for k, nprobe in ((10, 4), (100, 16), (7, 40)):
                    _both_modes(g, lists, cc, x, k, nprobe, lo, hi, filt=f, range_filters=rf,
                                what="ranges %s window %s %s" % (ranges is not None, lo, hi))
        g.binivf_set_scan_mode(1)
        # the default window excludes an exact duplicate (Hamming 0), [0, 1e4] keeps it
        D, I = g.binivf_search(x, 5, _args(nlist))
        assert (D > 0).all()
        D, I = g.binivf_search(x, 5, _args(nlist, 0, 1e4))
        assert (D[:, 0] == 0).all()
    finally:
        g.close()


def test_the_same_heap_operations(edges):
    """admissions under mode 1 == under mode 0 == the restated serial scan's"""
    g, lists, cc, x = edges
    for k, nprobe in ((1, 8), (10, 3), (100, 8), (300, 8)):
        want = SR.counts(lists, cc, x, k, nprobe, C, 0, 1e4)
        got = []
        for mode in (1, 0):
            g.binivf_set_scan_mode(mode)
            g.profile_enable(1)
            g.binivf_stats(reset=True)
            g.binivf_scan_stats(reset=True)
            g.binivf_search(x, k, _args(nprobe, 0, 1e4))
            got.append(g.binivf_stats(reset=True))
            st = g.binivf_scan_stats(reset=True)
            g.profile_enable(0)
            assert st == ((x.shape[0], want[2], want[1], 0) if mode == 1 else (0, 0, 0, 0)), (k, nprobe, mode, st, want)
        assert got[0] == got[1] == (x.shape[0], want[0]), (k, nprobe, got, want)


def test_fallback_under_a_small_budget(edges):
    g, lists, cc, x = edges
    ref = BR.search(lists, cc, x, 10, 8, 0, 1e4)
    g.binivf_set_scan_mode(1)
    try:
        g.set_dist_budget(4096)
        st = _spread_queries(g, lambda: _same(*g.binivf_search(x, 10, _args(8, 0, 1e4)), *ref, "small budget"))
        assert st == (0, 0, 0, x.shape[0])
    finally:
        g.set_dist_budget(BIG)
    st = _spread_queries(g, lambda: _same(*g.binivf_search(x, 10, _args(8, 0, 1e4)), *ref, "budget restored"))
    assert st[0] == x.shape[0] and st[3] == 0


def test_device_entry_and_realtime_add():
    nbits, nlist = 96, 16
    allc = BR.clustered_codes(5000, nbits, 10, flip=0.05, seed=31, dup_frac=0.1)
    cc = BR.train(allc[:nlist * 40], nlist)
    g = api.GammaHip(0)
    try:
        g.binivf_init(nbits, nlist, bucket_init_size=50)   # small buckets: the lists grow between the searches
        g.binivf_set_trained(cc)
        g.binivf_set_scan_mode(1)
        x = np.ascontiguousarray(allc[::250])
        nq, k = x.shape[0], 20
        dx = torch.from_numpy(x).cuda()
        dD = torch.empty((nq, k), dtype=torch.float32, device="cuda")
        dI = torch.empty((nq, k), dtype=torch.int64, device="cuda")
        lists, first = None, 0
        for m in (1500, 3500):   # the second search sees the second add
            g.binivf_add(allc[first:first + m], first)
            lists = BR.assign_lists(allc[first:first + m], cc, first, lists)
            first += m
            Dr, Ir = BR.search(lists, cc, x, k, 6, 0, 1e4)
            st = _spread_queries(g, lambda: (g.binivf_search_device(dx.data_ptr(), nq, k, _args(6, 0, 1e4), dD.data_ptr(),
                                                                    dI.data_ptr()), torch.cuda.synchronize()))
            assert st[0] == nq and st[3] == 0
            _same(dD.cpu().numpy(), dI.cpu().numpy(), Dr, Ir, "device entry after %d rows" % first)
            D, I = g.binivf_search(x, k, _args(6, 0, 1e4))
            _same(D, I, Dr, Ir, "host entry after %d rows" % first)
    finally:
        g.close()


def test_switches(edges):
    g, lists, cc, x = edges
    assert AUTO_MAX_NQ >= 0 and C > 0
    fresh = api.GammaHip(0)
    try:
        fresh.binivf_init(64, 4)
        assert fresh.binivf_scan_mode() == -1   # the default
    finally:
        fresh.close()
    for bad in (2, -2, 7):
        with pytest.raises(api.GammaHipError):
            g.binivf_set_scan_mode(bad)
    fl = api.GammaHip(0)   # a float model's handle
    try:
        fl.raw_init(16)
        fl.ivfflat_init(16, 4)
        with pytest.raises(api.GammaHipError):
            fl.binivf_set_scan_mode(1)
        with pytest.raises(api.GammaHipError):
            fl.binivf_scan_stats()
    finally:
        fl.close()
    for mode in (0, 1, -1):
        g.binivf_set_scan_mode(mode)
        assert g.binivf_scan_mode() == mode
    # mode -1: a call of auto_max_nq + 1 queries is not spread; one of auto_max_nq (if any) is
    n = AUTO_MAX_NQ + 1
    xs = np.ascontiguousarray(np.resize(x, (n, x.shape[1])))   # the queries of x over and over: row i is x[i % len(x)]
    ref = tuple(np.resize(a, (n, 10)) for a in BR.search(lists, cc, x, 10, 3, 0, 1e4))
    st = _spread_queries(g, lambda: _same(*g.binivf_search(xs, 10, _args(3, 0, 1e4)), *ref, "auto, beyond"))
    assert st == (0, 0, 0, 0)
    if AUTO_MAX_NQ > 0:
        st = _spread_queries(g, lambda: _same(*g.binivf_search(xs[:AUTO_MAX_NQ], 10, _args(3, 0, 1e4)),
                                              ref[0][:AUTO_MAX_NQ], ref[1][:AUTO_MAX_NQ], "auto, within"))
        assert st[0] == AUTO_MAX_NQ


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, %r)
from gamma_amd import api
from tests import binivf_ref as BR
base = BR.clustered_codes(600, 64, 4, seed=1)
g = api.GammaHip(0)
g.binivf_init(64, 4)
g.binivf_set_trained(base[:4])
g.binivf_add(base, 0)
g.binivf_set_scan_mode(1)
g.profile_enable(1)
D, I = g.binivf_search(base[:3], 5, api.SearchArgs(nprobe=2, min_score=0, max_score=1e4))
Dr, Ir = BR.search(BR.assign_lists(base, base[:4]), base[:4], base[:3], 5, 2, 0, 1e4)
assert np.array_equal(I, Ir) and D.tobytes() == Dr.tobytes()
print("SPREAD", g.binivf_scan_stats()[0], g.binivf_stats()[0])
g.close()
"""


def test_environment_switch():
    """GAMMA_HIP_NO_BIN_SPREAD=1 in a fresh process: mode 1 runs as mode 0"""
    for env_on, want in ((True, "SPREAD 0 3"), (False, "SPREAD 3 3")):
        env = dict(os.environ)
        env.pop("GAMMA_HIP_NO_BIN_SPREAD", None)
        if env_on:
            env["GAMMA_HIP_NO_BIN_SPREAD"] = "1"
        out = subprocess.run([sys.executable, "-c", _CHILD % ROOT], env=env, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr[-2000:]
        assert want in out.stdout, out.stdout
