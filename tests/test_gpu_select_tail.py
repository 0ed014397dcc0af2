"""The tail of the bounded scan: k_select_final's sorting network over the wave's <= 256 (512) items, its early gather, and the
fall-through chain (unfiltered selection, tie-cut flags, id look-ups) driven from the list of fallen-through queries.

Every case is the smallest shape at which the bounded scan and its byte-image consumers are on -- 520 queries x 32 probes over
64 lists, d 32, M 16 -- and compares the whole search (probed lists, recall-stage tables, final results) with the oracle,
bit for bit.  The data is integer-valued (synth.sift_like), so equal ADC keys at different positions occur: the order inside
them is by position."""
import numpy as np
import pytest

from gamma_amd import api, synth
from oracle import binding as B
from tests import fixtures
from tests.parity import compare_search_exact
from tests.test_gpu_more import run_both

pytestmark = pytest.mark.gpu
NQ, P = 520, 32


def _first_group_sizes(case, q):
    """Candidates of every query's first probe group: the lengths of its four nearest lists (32 probes in 8 groups)."""
    lens = np.array([len(case["oracle"].get_list(l)[0]) for l in range(case["nlist"])])
    d2 = ((q.astype(np.float64)[:, None, :] - case["cc"].astype(np.float64)[None, :, :]) ** 2).sum(2)
    return lens[np.argsort(d2, axis=1, kind="stable")[:, :4]].sum(1)


@pytest.fixture(scope="module")
def tail():
    """N = 24000: a first probe group (4 probes x ~375 codes) of fewer than 2048 candidates, for every query."""
    case = fixtures.trained_case(d=32, nlist=64, M=16, N=24000, nq=24, metric=B.METRIC_L2)
    q = synth.sift_like(NQ, d=32, seed=4242)
    first = _first_group_sizes(case, q)
    assert (first <= 2048).all(), first.max()
    g = fixtures.load_hip(case)
    g.set_scan_bound_feedback(False)   # every call of this module takes the bounded scan, whatever fell through before
    yield case, g, q
    g.close()


_last_kind = {}   # handle -> the kind of its last call


def _check(case, g, q, R, metric, has_rank, del_bm=None):
    """One search on both sides; returns how many queries took the bounded scan and how many of them fell through.
    The handle keeps these counters per kind of call (nprobe, recall_num, metric, filter clause; gamma_hip_search.cpp) and
    starts a new kind from zero: the first call of a kind reads them as they stand, a repeated kind takes the difference.
    Either way the count of queries is asserted, so a wrong reading cannot pass for another quantity."""
    kind = (R, metric, del_bm is not None)
    fresh = _last_kind.get(id(g)) != kind
    _last_kind[id(g)] = kind
    s0 = g.scan_bound_stats()
    k = min(10, R)
    (D, I, st), (Dg, Ig) = run_both(case, g, q, k, P, R, metric, has_rank, coarse_mode=1, del_bitmap=del_bm)
    sg = g.last_stages(len(q), P, R)
    s1 = g.scan_bound_stats()
    compare_search_exact(D, I, st, Dg, Ig, sg)
    base = dict(queries=0, fell_through=0) if fresh else s0
    return s1["queries"] - base["queries"], s1["fell_through"] - base["fell_through"]


@pytest.mark.parametrize("has_rank", [True, False])
@pytest.mark.parametrize("R", [1, 63, 64, 65, 128, 200, 255, 256, 300])
def test_select_final_at_the_run_boundaries(tail, R, has_rank):
    """recall_num at the network's row boundaries (a lane holds items 64 apart): one item, one short of a row, a full row, one
    more, two rows, a ragged fourth row, a full network; 300 takes the eight-row kernel."""
    case, g, q = tail
    queries, fell = _check(case, g, q, R, B.METRIC_L2, has_rank)
    print("recall_num %d: %d queries through the bounded scan, %d fell through" % (R, queries, fell))
    assert queries == NQ


def test_no_query_falls_through_on_ordinary_data(tail):
    """The fall-through launches find an empty list and must leave every row alone."""
    case, g, q = tail
    queries, fell = _check(case, g, q, 100, B.METRIC_L2, True)
    assert queries == NQ and fell == 0


def test_inner_product_takes_the_same_selection(tail):
    """Inner product: no byte image, the same selection kernels on the complemented keys."""
    case, g, q = tail
    for has_rank in (True, False):
        queries, _ = _check(case, g, q, 100, B.METRIC_IP, has_rank)
        assert queries == NQ


def test_first_group_with_fewer_than_recall_num_valid_entries(tail):
    """90 % deleted: first groups hold fewer than recall_num valid entries, those queries have no bound and are listed for the
    unfiltered selection; the others go through the network with rows that are partly padding."""
    case, g, q = tail
    N = case["N"]
    rng = np.random.default_rng(5)
    dead = rng.choice(N, size=int(N * 0.9), replace=False)
    bm = np.zeros((N >> 3) + 1, dtype=np.uint8)
    np.bitwise_or.at(bm, dead >> 3, (1 << (dead & 7)).astype(np.uint8))
    g.bitmap_upload(bm, N)
    case["oracle"].set_docids_bitmap(bm)
    try:
        for R in (120, 256):
            for has_rank in (True, False):
                queries, fell = _check(case, g, q, R, B.METRIC_L2, has_rank, del_bm=bm)
                print("90 %% deleted, recall_num %d: %d of %d fell through" % (R, fell, queries))
                assert queries == NQ and fell > 0
    finally:
        case["oracle"].set_docids_bitmap(np.zeros((N >> 3) + 1, dtype=np.uint8))
        g.bitmap_upload(np.zeros(1, dtype=np.uint8), 0)


def test_first_group_longer_than_one_round():
    """N = 48000: a first probe group (the query's four nearest lists) of ~3000 candidates, more than one 2048-item round of
    the producer's epilogue, for every query of the batch (the module's other cases: ~1500, one round)."""
    case = fixtures.trained_case(d=32, nlist=64, M=16, N=48000, nq=24, metric=B.METRIC_L2)
    g = fixtures.load_hip(case)
    try:
        g.set_scan_bound_feedback(False)
        q = synth.sift_like(NQ, d=32, seed=4243)
        first = _first_group_sizes(case, q)
        assert (first > 2048).all(), first.min()
        for R in (100, 256):
            queries, _ = _check(case, g, q, R, B.METRIC_L2, True)
            assert queries == NQ
    finally:
        g.close()


def _dup_index(base, d, nlist, M):
    from tests import lloyd as train
    cc, pq = train.train_ivfpq(base[:6000], nlist, M, niter=6, pq_niter=8, seed=9, device="cpu")
    o = B.OracleIVFPQ(d, nlist, M, 8, B.METRIC_L2, bucket_init_size=4000)
    o.set_trained(cc, pq, None)
    B.lib().go_set_assign_mode(1)
    assert o.add(base)
    B.lib().go_set_assign_mode(0)
    o.set_raw(base)
    g = api.GammaHip(0)
    g.ivfpq_init(d, nlist, M, 8, api.METRIC_L2, 4000)
    g.ivfpq_set_trained(cc, pq, None)
    g.add(base, 0)
    g.raw_init(d)
    g.raw_append(base)
    g.set_scan_bound_feedback(False)
    return dict(oracle=o), g


def test_some_queries_fall_through_and_the_listed_launches_finish_them():
    """Six base vectors with 600 copies each among ordinary ones: a query that sits on one of them meets more equal keys than
    the network holds (or than a slice holds) and is handed to the repair scan and the listed launches -- unfiltered selection,
    tie-cut flags, id look-ups; the ordinary queries of the batch stay on the bounded path."""
    d, nlist, M, N = 32, 64, 16, 24000
    rng = np.random.default_rng(3)
    distinct = synth.sift_like(6, d=d, seed=77)
    base = synth.sift_like(N, d=d, seed=78)
    rows = rng.choice(np.arange(6000, N), size=3600, replace=False)   # (the training sample stays ordinary)
    base[rows] = distinct[np.arange(3600) % 6]
    q = np.concatenate([np.tile(distinct, (10, 1)), synth.sift_like(NQ - 60, d=d, seed=79)])
    case, g = _dup_index(base, d, nlist, M)
    try:
        for R in (120, 300):
            for has_rank in (True, False):
                queries, fell = _check(case, g, q, R, B.METRIC_L2, has_rank)
                print("six vectors x 600 copies, recall_num %d: %d of %d fell through" % (R, fell, queries))
                assert queries == NQ
                assert 0 < fell < queries
    finally:
        g.close()


def test_every_query_falls_through():
    """Sixty distinct vectors, 400 copies each (the construction of test_scan_bound_fallback_paths): the whole batch is listed,
    more rows than the listed launches have workgroups, so these stride over the list."""
    d, nlist, M, N = 32, 64, 16, 24000
    rng = np.random.default_rng(3)
    distinct = synth.sift_like(60, d=d, seed=77)
    base = distinct[rng.integers(0, 60, size=N)].copy()
    base[:2000] = synth.sift_like(2000, d=d, seed=78)
    q = np.concatenate([distinct[:60], synth.sift_like(NQ - 60, d=d, seed=79)])
    case, g = _dup_index(base, d, nlist, M)
    try:
        queries, fell = _check(case, g, q, 256, B.METRIC_L2, True)
        print("sixty vectors x 400 copies, recall_num 256: %d of %d fell through" % (fell, queries))
        assert queries == NQ and fell > 256
    finally:
        g.close()
