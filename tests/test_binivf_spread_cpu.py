"""CPU: what the spread scan of the binary IVF model rests on (gamma_amd/csrc/binivf_spread.hip), at the value level.

A query's row sequence is its probed lists in coarse order, each list in list order.  Cut it into chunks of C rows that never
span two lists and let B_c be the k-th smallest valid distance of the rows before chunk c (no bound while fewer than k).
The serial heap's top before any row of chunk c is <= B_c and never rises, so feeding only the rows with dis < B_c through
`dis < top -> heap_pop + heap_push`, in sequence order, gives the result of feeding every valid row -- the same (values, ids)
at EVERY rank, order inside ties included -- and admits the same rows.  Checked through the oracle's heap stream and, where
oracle/_ref exists, the compiled faiss heaps."""
import numpy as np
import pytest

from oracle import binding as B
from tests import binflat_ref as BF
from tests import binivf_ref as BR
from tests import binivf_spread_ref as SR

need_ref = pytest.mark.skipif(not B.have_ref(), reason="oracle/_ref not built (needs the reference tree)")

ORDERS = ("random", "ascending", "descending", "equal")


def _lists(order, nbits, lens, seed):
    """lists of the given lengths whose concatenation, in list order, has its distances to the query in the given order;
    returns (lists, query)"""
    rng = np.random.default_rng(seed)
    cs = nbits // 8
    n = int(sum(lens))
    q = rng.integers(0, 256, cs, dtype=np.uint8)
    codes = rng.integers(0, 256, (n, cs), dtype=np.uint8)
    d = BR.hamming(q, codes)
    if order == "ascending":
        codes = codes[np.argsort(d, kind="stable")]
    elif order == "descending":
        codes = codes[np.argsort(-d, kind="stable")]
    elif order == "equal":
        codes[:] = codes[0]
    vids = rng.permutation(n).astype(np.int64)   # labels unrelated to positions
    lists, at = [], 0
    for m in lens:
        lists.append((vids[at:at + m], np.ascontiguousarray(codes[at:at + m])))
        at += m
    return lists, q


def _check(lists, probes, q, k, C, use_ref=False, filt=None, lo=0, hi=1e4):
    vals, ids, chunk, nch, _ = SR.sequence(lists, probes, q, C, lo, hi, filt)
    assert nch == sum(SR.chunk_counts([lists[l][0].size if l >= 0 else 0 for l in probes], C))
    cand = SR.candidates(vals, chunk, k, nch)
    adm = BF.admitted(vals, k)
    assert not (adm & ~cand).any()                                  # every admitted row is a candidate
    assert np.array_equal(BF.admitted(vals[cand], k), adm[cand])    # the replay admits the same rows: as many admissions
    fv, fi = BR.heap_pop_push_stream(vals, ids, k, use_ref)
    cv, ci = BR.heap_pop_push_stream(vals[cand], ids[cand], k, use_ref)
    assert np.array_equal(fi, ci) and fv.tobytes() == cv.tobytes()
    return cand, chunk


def _edge_lens(C):
    return [0, 1, max(C - 1, 0), C, C + 1, 0, 3 * C + 5, 200]


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("nbits", [8, 256])   # nine distinct distances; a spread
@pytest.mark.parametrize("k", [1, 10, 100])
def test_replaying_the_candidates_is_replaying_the_sequence(order, nbits, k):
    for C in (1, 3, 64):
        lens = _edge_lens(C)
        lists, q = _lists(order, nbits, lens, nbits + k + C)
        probes = np.array([6, 3, -1, 0, 4, 1, 7, 2, 5, -1])   # a -1 slot inside and at the end; lists of 0, 1, C - 1, C, C + 1
        _check(lists, probes, q, k, C)
        _check(lists, probes[:1], q, k, C)


@need_ref
@pytest.mark.parametrize("order", ORDERS)
def test_replaying_the_candidates_on_the_compiled_heaps(order):
    lists, q = _lists(order, 256, _edge_lens(64), 9)
    for k in (1, 10, 100):
        _check(lists, np.array([6, 3, -1, 0, 4, 1, 7, 2, 5]), q, k, 64, use_ref=True)


def test_a_chunk_without_a_valid_row():
    """a filter that invalidates every row of one chunk (and a score window that drops others): the chunk counts nothing,
    bounds and candidates are over the valid rows only"""
    C, k = 64, 10
    lists, q = _lists("random", 256, [C + 1, 3 * C + 5, C], 2)
    dead = lists[1][0][C:2 * C]                       # chunk 1 of list 1
    f = BR.Filter(deleted=dead)
    probes = np.array([1, 0, 2])
    cand, chunk = _check(lists, probes, q, k, C, filt=f)
    assert not (chunk == 1).any() and (chunk == 0).any() and (chunk == 2).any()
    d = BR.hamming(q, lists[1][1])
    _check(lists, probes, q, k, C, filt=f, lo=float(np.median(d)), hi=1e4)
    _check(lists, probes, q, k, C, filt=f, lo=1e5, hi=2e5)    # nothing valid at all


def test_first_chunks_have_no_bound_and_descending_rows_are_all_candidates():
    C, k = 64, 10
    lists, q = _lists("descending", 256, [5, 3 * C + 5, C], 3)
    vals, ids, chunk, nch, rows = SR.sequence(lists, np.array([0, 1, 2]), q, C, 0, 1e4)
    cand = SR.candidates(vals, chunk, k, nch)
    assert cand[chunk <= 1].all()          # 5 + 64 rows before chunk 2: chunks 0 and 1 see fewer than k, or k of the largest
    strictly = np.concatenate([[True], vals[1:] < vals[:-1]])
    assert cand[strictly].all()            # a row strictly below everything before it is always a candidate
    lists, q = _lists("equal", 256, [5, 3 * C + 5, C], 3)
    vals, ids, chunk, nch, rows = SR.sequence(lists, np.array([0, 1, 2]), q, C, 0, 1e4)
    cand = SR.candidates(vals, chunk, k, nch)
    assert cand.sum() == (chunk <= 1).sum()   # equal rows: once k precede a chunk, none of it is below the bound


def test_sequence_is_the_yardsticks_stream():
    """SR.sequence + the heap stream is tests/binivf_ref.py::search"""
    nbits, nlist = 64, 8
    base = BR.clustered_codes(1500, nbits, 6, seed=5, dup_frac=0.2)
    cc = base[:nlist].copy()
    lists = BR.assign_lists(base, cc)
    x = base[::300].copy()
    f = BR.Filter(deleted=np.arange(0, 1500, 5))
    for nprobe in (3, 0):   # 0: the model's 20 > nlist, -1 slots
        P = BR.resolve_nprobe(nprobe, nlist)
        _, probes = BR.coarse(x, cc, P)
        Dr, Ir = BR.search(lists, cc, x, 10, nprobe, 0, 1e4, filt=f)
        for r in range(x.shape[0]):
            vals, ids, chunk, nch, _ = SR.sequence(lists, probes[r], x[r], 64, 0, 1e4, f)
            cand = SR.candidates(vals, chunk, 10, nch)
            sv, si = BR.heap_pop_push_stream(vals[cand], ids[cand], 10)
            assert np.array_equal(si, Ir[r]) and np.where(si < 0, BR.EMPTY_D, sv).tobytes() == Dr[r].tobytes()
