"""GPU: the three scans of a wide IVFPQ handle (65 .. 256 sub-quantizers) -- the pair scan k_ivfpq_scan_wide, the list-major scan
k_ivfpq_scan_wide_lm behind ivfpq_wide_set_lm_scan, the table-mode-0 scan k_ivfpq_scan_wide_res -- at the shapes their other
tests (one recipe: an L2 index of 8 lists of ~625 codes, nprobe 4, k 10) never reach:
  a. lists of 0, 1, 255, 256, 257, 511, 512, 513, 1025, 0, 64 and 63 codes (the pair kernel's tile of 512 with the sums kept in
     registers or parked, the list-major slab of 256, lists nobody fills), nprobe 1 and 12, k and recall_num on both sides of
     each other, deletes + a range filter, a score window; 1000 inner-product queries at nprobe 12, where a workgroup's
     segment of two probes is often an empty list beside a list of one tile.  Under the filter variants the 64-query
     calls scan compacted shadow lists (compact_lists_for_call: the lengths are no longer the boundaries, the predicate is
     applied ahead of the scan); the calls of 1 and 3 queries scan the lists themselves and reach the kernels' id predicates
     at the boundary lengths;
  b. more work units than twice the list-major kernel's persistent grid: every workgroup walks several units;
  c. a workspace budget that cuts one call into several sub-batches with a ragged last one, on tie-heavy data;
  d. an inner-product index;
  e. a float16 raw store under a wide handle.
Strictly against the CPU oracle: compare_search_exact, exact ties on, no query excluded.  The pair and list-major handles are
held to the oracle with its precomputed table, the mode-0 handle's L2 searches to an oracle created under a lowered table limit
(its distances differ in their bits), inner-product searches of all three to the first.  tests/test_pqwide_recipes_cpu.py
asserts on the CPU that the inputs (tests/pqwide_recipes.py) are what is claimed here."""
import numpy as np
import pytest

from gamma_amd import api
from oracle import binding as B
from tests import pqwide_recipes as R
from tests.parity import compare_exact, compare_search_exact
from tests.test_gpu_mode0 import table_limit   # the oracle's and the device library's limit together, restored afterwards

pytestmark = pytest.mark.gpu
METRICS = (B.METRIC_L2, B.METRIC_IP)


def new_handle(st, mode0=False, bucket=1000):
    g = api.GammaHip(0)
    g.ivfpq_wide_init(st["d"], st["nlist"], st["M"], st["metric"], bucket, table_mode0=mode0)
    g.ivfpq_set_trained(st["cc"], st["pq"], None)
    return g


def load_lists(g, o, nlist):
    """the oracle's lists in one add_keys_batch"""
    lists = [(l,) + o.get_list(l) for l in range(nlist)]
    lists = [t for t in lists if len(t[1])]
    g.add_keys_batch([t[0] for t in lists], [len(t[1]) for t in lists], np.concatenate([t[1] for t in lists]),
                     np.concatenate([t[2] for t in lists]))


def device_search(g, q, call, filt=None):
    """tests/pqwide_recipes.py's oracle_search on the device: (D, I, stages of the call's last sub-batch)"""
    f = filt or {}
    rf = [api.make_range_filter(f["docs"], b_not_in=f.get("not_in", False))] if f.get("docs") is not None else None
    args = api.SearchArgs(metric=call["metric"], nprobe=call["P"], recall_num=call["R"], has_rank=call["has_rank"],
                          min_score=f.get("lo", -3e38), max_score=f.get("hi", 3e38), range_filters=rf)
    D, I = g.ivfpq_search(q, call["k"], args)
    return D, I, g.last_stages(len(q), call["P"], max(call["R"], call["k"]))


def check(expected, g, q, call, filt=None):
    D, I, st = expected
    Dg, Ig, sg = device_search(g, q, call, filt)
    compare_search_exact(D, I, st, Dg, Ig, sg)
    return Dg.tobytes(), Ig.tobytes()


def lm_serves(M):
    return api.ivfpq_wide_lm_shape(M)[0] != 0


def close_all(handles):
    for g in handles:
        g.close()


# ---- a. lists at the boundaries -------------------------------------------------------------------------------------------------
_edge_handles = {}


@pytest.fixture(scope="module")
def edge_handles():
    yield _edge_handles
    for _, _, gs in _edge_handles.values():
        close_all(gs)
    _edge_handles.clear()


def _edge(M, filtered, cache):
    """(state, mode-0 oracle, [pair handle, handle with the list-major switch on, mode-0 handle]) of an M, built once -- and
    once more for the variants that set delete bits: a handle that has ever held one takes the compacted-shadow-list path
    from then on, so the plain and window variants keep handles that never did and run the same path in any order"""
    if (M, filtered) not in cache:
        st = R.edge_state(M)
        with table_limit(st["nlist"] * M * 1024 - 1):
            o0 = R.edge_fill(B.OracleIVFPQ(st["d"], st["nlist"], M, 8, B.METRIC_L2), st)
            assert o0.use_precomputed_table() == 0
            g0 = new_handle(st, mode0=True)
        gp, gl = new_handle(st), new_handle(st)
        gl.ivfpq_wide_set_lm_scan(1)
        assert g0.use_precomputed_table() == 0 and gp.use_precomputed_table() == 1
        for g in (gp, gl, g0):
            g.raw_init(st["d"])
            g.raw_append(st["base"])
            for l, keys in enumerate(st["keys"]):   # one list per call; the empty lists get none
                if len(keys):
                    g.add_keys(l, keys, st["codes"][keys])
            assert [g.list_size(l) for l in range(st["nlist"])] == R.EDGE_LENS
        cache[(M, filtered)] = (st, o0, [gp, gl, g0])
    return cache[(M, filtered)]


@pytest.mark.parametrize("variant", R.EDGE_VARIANTS)
@pytest.mark.parametrize("M", R.EDGE_M)
def test_lists_at_the_boundaries(edge_handles, M, variant):
    filtered = variant.startswith("filter")
    st, o0, (gp, gl, g0) = _edge(M, filtered, edge_handles)
    o1 = st["oracle"]
    calls0 = gl.ivfpq_wide_lm_stats()[0]
    if filtered:
        for g in (gp, gl, g0):
            g.bitmap_set(st["deleted"])
    try:
        n = 0
        for call in R.edge_calls() + ([R.EDGE_BIG_CALL] if variant == "plain" else []):
            q = (st["q"] if call["nq"] <= 64 else st["q_big"])[:call["nq"]]
            filt = R.edge_filter(st, variant, call)
            want1 = R.oracle_search(o1, q, call, filt)
            want0 = R.oracle_search(o0, q, call, filt) if call["metric"] == B.METRIC_L2 else want1
            a = check(want1, gp, q, call, filt)
            assert check(want1, gl, q, call, filt) == a, call
            check(want0, g0, q, call, filt)
            n += 1
    finally:
        if filtered:
            for g in (gp, gl, g0):
                g.bitmap_set(st["deleted"], 0)
    # the switch engages where the kernel serves M, once per call; at M = 65 it is set and nothing engages
    assert gl.ivfpq_wide_lm_stats()[0] == calls0 + (n if lm_serves(M) else 0)
    assert lm_serves(M) or gl.ivfpq_wide_lm_stats() == (0, -1, 0)
    assert gp.ivfpq_wide_lm_stats() == (0, -1, 0)
    for g in (gp, gl, g0):
        assert g.ties_not_honoured() == 0


# ---- b. more units than the list-major grid --------------------------------------------------------------------------------------
def test_every_workgroup_of_the_list_major_grid_walks_several_units():
    from tests.test_gpu_pqwide import _handle
    case, q = R.units_case()
    o = case["oracle"]
    g = _handle(case)
    try:
        g.ivfpq_wide_set_lm_scan(1)
        on = []
        for metric in METRICS:
            call = dict(k=10, P=4, R=50, metric=metric, has_rank=True)
            want = R.oracle_search(o, q, call)
            units = R.lm_units(R.list_lens(o, 8), want[2]["coarse_idx"])
            assert units > 2 * R.LM_GRID, units
            on.append(check(want, g, q, call))
        assert g.ivfpq_wide_lm_stats() == (2, -1, 2 * len(q) * 4)
        g.ivfpq_wide_set_lm_scan(0)
        off = [device_search(g, q, dict(k=10, P=4, R=50, metric=metric, has_rank=True)) for metric in METRICS]
        assert g.ivfpq_wide_lm_stats()[0] == 2
        assert [(D.tobytes(), I.tobytes()) for D, I, _ in off] == on
        assert g.ties_not_honoured() == 0
    finally:
        g.close()


# ---- c. several sub-batches per call ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["pair", "list_major", "mode0"])
def test_a_call_cut_into_sub_batches(which):
    from tests.test_gpu_pqwide import _handle
    from tests.test_gpu_pqwide_mode0 import _mode0
    case, base, q = R.ties_case()
    if which == "mode0":
        o, g = _mode0(case, base)
    else:
        o = R.ties_oracle(case, base)
        g = _handle(case, base, o)
        if which == "list_major":
            g.ivfpq_wide_set_lm_scan(1)
    nq, P = len(q), 4
    try:
        lens = R.list_lens(o, 8)
        assert g.max_list_len() == max(lens)
        budget = R.ties_budget(lens, P)
        calls = [dict(k=10, P=P, R=10, metric=B.METRIC_L2, has_rank=True), dict(k=10, P=P, R=10, metric=B.METRIC_L2, has_rank=False),
                 dict(k=10, P=P, R=10, metric=B.METRIC_IP, has_rank=True)]
        for call in calls:
            want = R.oracle_search(o, q, call)
            whole = check(want, g, q, call)           # one chunk: every stage of every query
            chunk = R.scan_chunk(budget, lens, want[2]["coarse_idx"], 96,
                                 table_limited=not (which == "mode0" and call["metric"] == B.METRIC_L2))
            nchunks, last = -(-nq // chunk), nq - (nq - 1) // chunk * chunk
            assert nchunks >= 3 and last < chunk, (chunk, nchunks, last)
            c0 = g.ivfpq_wide_lm_stats()[0]
            g.set_dist_budget(budget)
            try:
                Dg, Ig, sg = device_search(g, q, call)
            finally:
                g.set_dist_budget(R.BIG_BUDGET)
            if which == "list_major":   # one launch, with an inverse index of its own, per sub-batch
                assert g.ivfpq_wide_lm_stats()[0] - c0 == nchunks, (g.ivfpq_wide_lm_stats(), c0, nchunks)
            compare_exact(want[0], want[1], Dg, Ig)
            assert (Dg.tobytes(), Ig.tobytes()) == whole
            # the stages the handle keeps are those of the call's last sub-batch: the ragged one
            compare_search_exact(want[0][nq - last:], want[1][nq - last:], {k: v[nq - last:] for k, v in want[2].items()},
                                 Dg[nq - last:], Ig[nq - last:], {k: v[:last] for k, v in sg.items()})
        assert g.ties_not_honoured() == 0
    finally:
        g.close()


# ---- d. an inner-product index -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [65, 128])
def test_an_inner_product_index(M):
    st = R.ip_case(M)   # (lists of several hundred codes each: tests/test_pqwide_recipes_cpu.py)
    d, nlist, base, q, o = st["d"], st["nlist"], st["base"], st["q"], st["oracle"]
    handles = [new_handle(st), new_handle(st)]
    try:
        handles[1].ivfpq_wide_set_lm_scan(1)
        for g in handles:
            g.raw_init(d)
            g.raw_append(base)
            load_lists(g, o, nlist)
            assert g.use_precomputed_table() == 1 and o.use_precomputed_table() == 1   # the oracle keeps a table whatever the index metric
            assert g.ivfpq_table().tobytes() == o.table().tobytes(), "precomputed table"
        for metric in METRICS:
            for has_rank in (True, False):
                for k, P, Rn in ((10, 4, 50), (1, 1, 1), (33, 8, 7)):
                    call = dict(k=k, P=P, R=Rn, metric=metric, has_rank=has_rank)
                    want = R.oracle_search(o, q, call)
                    assert check(want, handles[0], q, call) == check(want, handles[1], q, call)
        assert handles[0].ivfpq_wide_lm_stats() == (0, -1, 0)
        assert handles[1].ivfpq_wide_lm_stats()[0] == (12 if lm_serves(M) else 0)
        for g in handles:
            assert g.ties_not_honoured() == 0
    finally:
        close_all(handles)


# ---- e. a float16 raw store under a wide handle ---------------------------------------------------------------------------------------
def test_a_float16_raw_store_under_a_wide_handle():
    from tests.test_gpu_rawf16 import gauss3, rounded   # data that fp16 changes; numpy's rounding is the definition
    M, d, nlist, N = 96, 192, 8, 3000
    rng = np.random.default_rng(4600)
    base, q = gauss3(N, d, 4601), gauss3(64, d, 4602)
    assert not np.array_equal(rounded(base), base)
    cc, pq = R.sampled_state(base, nlist, M, rng)
    st = dict(d=d, nlist=nlist, M=M, metric=B.METRIC_L2, cc=cc, pq=pq)

    def oracle():   # `add`s the fp32 base, re-ranks over the ROUNDED rows: only the store is rounded
        o = B.OracleIVFPQ(d, nlist, M, 8, B.METRIC_L2)
        o.set_trained(cc, pq, None)
        B.lib().go_set_assign_mode(0)
        assert o.add(base)
        o.set_raw(rounded(base))
        return o

    o1 = oracle()
    with table_limit(nlist * M * 1024 - 1):
        o0 = oracle()
        g0 = new_handle(st, mode0=True)
    handles = [new_handle(st), new_handle(st), g0]
    try:
        handles[1].ivfpq_wide_set_lm_scan(1)
        for g in handles:
            g.raw_init(d, "float16")
            assert g.raw_elem_bytes() == 2
            g.raw_append(base)
            load_lists(g, o1, nlist)
        for metric in METRICS:
            for k, P, Rn in ((10, 4, 50), (5, 8, 300)):
                call = dict(k=k, P=P, R=Rn, metric=metric, has_rank=True)
                want1 = R.oracle_search(o1, q, call)
                want0 = R.oracle_search(o0, q, call) if metric == B.METRIC_L2 else want1
                assert check(want1, handles[0], q, call) == check(want1, handles[1], q, call)
                check(want0, g0, q, call)
        assert handles[1].ivfpq_wide_lm_stats()[0] == 4
        for g in handles:
            assert g.ties_not_honoured() == 0
    finally:
        close_all(handles)
