"""CPU: what the exact Hamming (binary flat) search rests on (gamma_amd/csrc/binflat.hip), at the value level.

The serial scan admits row i iff dis_i < the heap's top, the top is the k-th smallest valid distance seen so far and never
rises.  Cut the rows into chunks and let B_c be the k-th smallest valid distance of the rows before chunk c (no bound while
fewer than k): every admitted row of chunk c has dis < B_c, and replaying only the rows with dis < B_c, in order, with the
replay's own `dis < top` test performs the same heap operations -- the same (values, ids) at EVERY rank, order inside ties
included.  Checked through the oracle's heap stream and, where oracle/_ref exists, the compiled faiss heaps."""
import ctypes as C

import numpy as np
import pytest

from gamma_amd import _lib, plugin
from oracle import binding as B
from tests import binflat_ref as BF
from tests import binivf_ref as BR

need_ref = pytest.mark.skipif(not B.have_ref(), reason="oracle/_ref not built (needs the reference tree)")

ORDERS = ("random", "ascending", "descending", "equal")


def _stream(order, nbits, n, seed):
    """distances of n rows of nbits-bit codes to one query, in the given row order"""
    rng = np.random.default_rng(seed)
    cs = nbits // 8
    codes = rng.integers(0, 256, (n, cs), dtype=np.uint8)
    q = rng.integers(0, 256, cs, dtype=np.uint8)
    d = BR.hamming(q, codes).astype(np.float32)
    if order == "ascending":
        d = np.sort(d)
    elif order == "descending":
        d = np.sort(d)[::-1].copy()
    elif order == "equal":
        d[:] = d[0]
    return d


def _check(order, nbits, k, chunk, use_ref):
    n = 10000
    vals = _stream(order, nbits, n, nbits + k)
    pos = np.arange(n, dtype=np.int64)
    cand = BF.candidates_of_stream(vals, pos, k, chunk, n)
    adm = BF.admitted(vals, k)
    assert not (adm & ~cand).any()             # every admitted row is a candidate
    assert cand[:min(chunk, n)].all()          # chunk 0 has no bound
    assert np.array_equal(BF.admitted(vals[cand], k), adm[cand])   # the replay admits the same rows
    fv, fi = BR.heap_pop_push_stream(vals, pos, k, use_ref)
    cv, ci = BR.heap_pop_push_stream(vals[cand], pos[cand], k, use_ref)
    assert np.array_equal(fi, ci) and fv.tobytes() == cv.tobytes()
    return int(cand.sum()), int(adm.sum())


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("nbits", [8, 256])   # nine distinct distances; a spread
@pytest.mark.parametrize("k", [1, 10, 100])
def test_replaying_the_candidates_is_replaying_the_stream(order, nbits, k):
    for chunk in (512, 4096):
        _check(order, nbits, k, chunk, False)


@need_ref
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("nbits", [8, 256])
def test_replaying_the_candidates_on_the_compiled_heaps(order, nbits):
    for k in (1, 10, 100):
        _check(order, nbits, k, 512, True)


def test_invalid_rows_are_outside_the_stream():
    """filtered rows and rows outside the score window take no part: bounds and candidates are over the valid rows, at
    their row positions"""
    rng = np.random.default_rng(4)
    n, k, chunk = 6000, 10, 512
    codes = rng.integers(0, 256, (n, 4), dtype=np.uint8)
    x = rng.integers(0, 256, (3, 4), dtype=np.uint8)
    dm = BF.hamming_matrix(x, codes)
    f = BR.Filter(deleted=rng.choice(n, 900, replace=False), ranges=[(np.arange(100, 5000), False)])
    for vals, vids in BF.valid_streams(dm, 6, 20, f):
        cand = BF.candidates_of_stream(vals, vids, k, chunk, n)
        assert not (BF.admitted(vals, k) & ~cand).any()
        a = BR.heap_pop_push_stream(vals, vids, k)
        b = BR.heap_pop_push_stream(vals[cand], vids[cand], k)
        assert np.array_equal(a[1], b[1]) and a[0].tobytes() == b[0].tobytes()


def test_yardstick_is_the_one_list_binivf_search():
    """tests/binflat_ref.py::search (distances from one matrix product) is tests/binivf_ref.py::search over ONE list that
    holds every code in vid order, nprobe 1"""
    for nbits, n in ((8, 700), (40, 900), (256, 1500)):
        codes = BR.clustered_codes(n, nbits, 6, flip=0.05, seed=nbits, dup_frac=0.2)
        x = np.ascontiguousarray(np.concatenate([codes[::211], BR.clustered_codes(5, nbits, 3, seed=1)]))
        dm = BF.hamming_matrix(x, codes)
        assert np.array_equal(dm, np.stack([BR.hamming(q, codes) for q in x]))
        f = BR.Filter(deleted=np.arange(0, n, 7), ranges=[(np.arange(50, n - 50), False), (np.arange(300, 400), True)],
                      vid2doc=np.arange(n) // 2 * 2)
        for filt in (None, f):
            for lo, hi in ((None, None), (0, 1e4), (1, 3), (1e5, 2e5)):
                for k in (1, 10, 1000):
                    a = BF.one_list(codes, x, k, lo, hi, filt)
                    b = BF.search(dm, k, lo, hi, filt)
                    assert np.array_equal(a[1], b[1]) and a[0].tobytes() == b[0].tobytes()
    a = BF.one_list(np.zeros((0, 8), np.uint8), np.zeros((2, 8), np.uint8), 3)   # an empty store: padding
    assert (a[1] == -1).all() and (a[0] == BR.EMPTY_D).all()


def test_design_candidate_count_of_the_stats_case_lies_under_its_cap():
    """the input of tests/test_gpu_binflat.py::test_stats: N = 2C + 37 random 256-bit rows, k = 10 -- the design's own
    candidate count lies inside admissions <= candidates <= C + N / 8 per query"""
    Cr = int(_lib.load().gamma_hip_binflat_chunk_rows())
    N = 2 * Cr + 37
    rng = np.random.default_rng(77)
    base = rng.integers(0, 256, (N, 32), dtype=np.uint8)
    x = rng.integers(0, 256, (7, 32), dtype=np.uint8)
    dm = BF.hamming_matrix(x, base)
    for r in range(7):
        cand = BF.design_candidates(dm[r:r + 1], 10, Cr, 0, 1e4)
        adm = BF.admissions(dm[r:r + 1], 10, 0, 1e4)
        assert adm <= cand <= Cr + N // 8, (r, adm, cand)


def test_brute_harness_entry():
    """gh_bin_search_brute takes gh_bin_search's arguments plus `int brute`, and parses the retrieval parameters as it does:
    a JSON that does not parse is refused (-100) before the model is asked"""
    assert plugin.BIN_SYMBOLS["gh_bin_search_brute"][1] == plugin.BIN_SYMBOLS["gh_bin_search"][1] + [C.c_int]
    L = plugin.load_host()
    h = L.gh_bin_new(b"HIPBINARYIVF", 8)
    assert h
    try:
        x = np.zeros((1, 8), np.uint8)
        D = np.zeros((1, 3), np.float32)
        I = np.zeros((1, 3), np.int64)
        one = (C.c_int * 1)(0)
        docs = np.zeros(1, np.int64)

        def call(fn, params, *tail):
            return fn(h, params, 0.0, 1e4, 1, x.ctypes.data_as(plugin.u8p), 3, D.ctypes.data_as(plugin.f32p),
                      I.ctypes.data_as(plugin.i64p), 0, docs.ctypes.data_as(plugin.i64p), one, one, *tail)

        for brute in (0, 1):
            assert call(L.gh_bin_search_brute, b"{\"nprobe\": ", brute) == -100
        assert call(L.gh_bin_search, b"{\"nprobe\": ") == -100
    finally:
        L.gh_bin_free(h)
