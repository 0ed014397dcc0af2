"""GPU: the list-major scan of a 4-bit handle (gamma_hip_ivfpq4_set_lm_scan, k_ivfpq4_scan_lm), switch on, against the yardstick
of tests/pq4_ref.py through compare_search_exact (exact ties on, no query excluded); the counters say which scan served a call."""
import threading

import numpy as np
import pytest

from gamma_amd import api
from oracle import binding as B
from tests import pq4_ref as PR
from tests.parity import compare_exact, compare_search_exact

pytestmark = pytest.mark.gpu

N, WIDE = 6000, dict(min_score=-3e38, max_score=3e38)
_cases = {}


def _case(d, nlist, M):
    key = (d, nlist, M)
    if key not in _cases:
        base = PR.clustered(N, d, 3)
        cc, pq = PR.train(base[:3000], nlist, M)
        B.lib().go_set_assign_mode(-1)
        lno, codes = PR.encode(base, cc, pq)
        _cases[key] = dict(d=d, nlist=nlist, M=M, base=base, cc=cc, pq=pq, lno=lno, codes=codes)
    c = _cases[key]
    return c, PR.Index(c["cc"], c["pq"], PR.build_lists(c["lno"], c["codes"], nlist), raw=c["base"].copy())


@pytest.fixture
def handle():
    made = []

    def make(c, add=True):
        g = api.GammaHip(0)
        made.append(g)
        g.ivfpq4_init(c["d"], c["nlist"], c["M"], api.METRIC_L2)
        g.ivfpq_set_trained(c["cc"], c["pq"], None)
        g.raw_init(c["d"])
        g.raw_append(c["base"])
        if add:
            g.add(c["base"], 0)
        g.ivfpq4_set_lm_scan(1)
        return g
    yield make
    [g.close() for g in made]


def _check(g, ix, q, k, P, R, has_rank=True, l2=True, filt=None, **kw):
    args = api.SearchArgs(metric=api.METRIC_L2 if l2 else api.METRIC_IP, nprobe=P, recall_num=R, has_rank=has_rank, **WIDE, **kw)
    c0, _, p0 = g.ivfpq4_lm_stats()
    Dg, Ig = g.ivfpq_search(q, k, args)
    sg = g.last_stages(q.shape[0], P, max(R, k))
    c1, _, p1 = g.ivfpq4_lm_stats()
    assert (c1 - c0, p1 - p0) == (1, q.shape[0] * P)   # served list-major: one launch of nq x nprobe pairs
    D, I, st = ix.search(q, k, P, recall_num=R, has_rank=has_rank, l2=l2, filt=filt, **WIDE)
    compare_search_exact(D, I, st, Dg, Ig, sg)
    assert g.ties_not_honoured() == 0
    return Dg, Ig, sg


@pytest.mark.parametrize("d, nlist, M", [(32, 16, 8), (128, 16, 32), (128, 16, 64), (64, 16, 16), (20, 16, 5), (24, 16, 12)])
def test_shapes(d, nlist, M, handle):
    c, ix = _case(d, nlist, M)
    lens = [ix.lists[l][0].size for l in range(nlist)]
    assert max(lens) > 512 and 0 < min(lens) <= 256, lens   # several slabs with a ragged last one, and a single slab
    g = handle(c)
    q = PR.clustered(64, d, 99)
    for l2 in (True, False):
        for has_rank in (True, False):
            _check(g, ix, q, 10, 6, 50, has_rank=has_rank, l2=l2)


@pytest.mark.parametrize("nq", [1, 3, 64, 4096])
def test_batch_sizes(nq, handle):
    c, ix = _case(32, 16, 8)
    g = handle(c)
    q = PR.clustered(nq, 32, 1000 + nq)
    for has_rank in (True, False):
        _check(g, ix, q, 10, 5, 40, has_rank=has_rank)


def test_an_empty_list_and_nprobe_beyond_nlist(handle):
    c, _ = _case(32, 16, 8)
    g = handle(c, add=False)
    keep = np.nonzero(c["lno"] != 0)[0]   # list 0 stays empty: every vector but those the yardstick assigns to it; all lists probed
    lists = [(keep[ids], cds) for ids, cds in PR.build_lists(c["lno"][keep], c["codes"][keep], 16)]
    g.add_keys_batch(range(1, 16), [x[0].size for x in lists[1:]], np.concatenate([x[0] for x in lists[1:]]),
                     np.concatenate([x[1] for x in lists[1:]]))
    q = PR.clustered(40, 32, 17)
    _check(g, PR.Index(c["cc"], c["pq"], lists, raw=c["base"].copy()), q, 10, 16, 50)
    # nprobe > nlist is refused at the entry: probes of -1 cannot reach the scan of a 4-bit handle (no shard entries)
    with pytest.raises(api.GammaHipError, match="nprobe"):
        g.ivfpq_search(q, 10, api.SearchArgs(metric=api.METRIC_L2, nprobe=17, recall_num=50, has_rank=True, **WIDE))


def test_deletes_filters_and_two_filters_in_one_tile(handle):
    c, ix = _case(32, 16, 8)
    rng, g = np.random.default_rng(8), handle(c)
    q = PR.clustered(48, 32, 6)
    deleted = rng.choice(N, N // 5, replace=False)
    g.bitmap_set(deleted)
    g.delete(deleted)
    _check(g, ix, q, 10, 6, 50, filt=PR.Filter(deleted=deleted))
    docs = rng.choice(N, N // 2, replace=False)
    for not_in in (False, True):
        _check(g, ix, q, 10, 6, 50, filt=PR.Filter(deleted=deleted, ranges=[(docs, not_in)]),
               range_filters=[api.make_range_filter(docs, b_not_in=not_in)])
    col = rng.integers(0, 100, N).astype(np.int32)   # device field filter: an int32 column, [lo, hi] inclusive
    g.field_append(0, col)
    _check(g, ix, q, 10, 6, 50, filt=PR.Filter(deleted=deleted, ranges=[(np.nonzero((col >= 20) & (col <= 60))[0], False)]),
           field_filters=[(0, 20, 60, True, True)])
    # two small host calls with different filters from two threads, combined: one tile carries two filter descriptors
    qs = [PR.clustered(5, 32, 300 + i) for i in range(2)]
    filts = [PR.Filter(deleted=deleted, ranges=[(docs, bool(i))]) for i in range(2)]
    want = [ix.search(qs[i], 10, 6, recall_num=50, coarse_mode=0, filt=filts[i], **WIDE)[:2] for i in range(2)]
    errors = []

    def client(i):
        try:
            args = api.SearchArgs(metric=api.METRIC_L2, nprobe=6, recall_num=50, has_rank=True, coarse_mode=0,
                                  range_filters=[api.make_range_filter(docs, b_not_in=bool(i))], **WIDE)
            for _ in range(20):
                compare_exact(want[i][0], want[i][1], *g.ivfpq_search(qs[i], 10, args))
        except BaseException as e:   # noqa: B902 (reported by the main thread)
            errors.append((i, repr(e)))

    th = [threading.Thread(target=client, args=(i,)) for i in range(2)]
    [x.start() for x in th]
    [x.join() for x in th]
    assert not errors, errors[:2]


def test_switch_semantics(handle):
    c, ix = _case(32, 16, 8)
    g, g8 = handle(c), api.GammaHip(0)
    q = PR.clustered(64, 32, 5)
    on = _check(g, ix, q, 10, 6, 50)            # (asserts calls + 1, pairs + nq * nprobe)
    before, was = g.ivfpq4_lm_stats(), g.ivfpq4_lm_scan()
    g.ivfpq4_set_lm_scan(0)
    Do, Io = g.ivfpq_search(q, 10, api.SearchArgs(metric=api.METRIC_L2, nprobe=6, recall_num=50, has_rank=True, **WIDE))
    so = g.last_stages(64, 6, 50)
    assert (was, g.ivfpq4_lm_scan()) == (1, 0) and g.ivfpq4_lm_stats() == before
    assert Do.tobytes() == on[0].tobytes() and Io.tobytes() == on[1].tobytes()
    assert all(so[k].tobytes() == on[2][k].tobytes() for k in so)
    g8.ivfpq_init(32, 16, 8)
    assert g8.L.gamma_hip_ivfpq4_set_lm_scan(g8.h, 1) == -6 and "4-bit" in g8.L.gamma_hip_last_error(g8.h).decode()   # EUNSUPPORTED
    g8.close()
    for M, mt in ((8, 8), (16, 16), (32, 32), (64, 64), (5, 0), (12, 0), (128, 0)):
        assert api.ivfpq4_lm_shape(M)[::2] == (mt, 2 * M * 16 * 4) and api.ivfpq4_lm_shape(M)[1] >= 1, M
