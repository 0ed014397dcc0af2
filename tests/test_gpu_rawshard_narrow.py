"""GPU: raw rows sharded with their lists in a NARROW store (gamma_hip_set_sparse_narrow_rows): the sparse
form of a float16 / uint8 / int8 / sq8 store, gamma_hip_ivfpq_shard_exact and _shard_export_exact over it, and the in-process
group on top.  Every member lives on device 0, as in tests/test_gpu_group_rawshard.py.

The contract is the narrow stores': a row is widened (sq8: decoded) exactly as it is loaded and every distance is fvec_L2sqr /
fvec_inner_product of the fp32 query and that row.  So every expected value here is that of an fp32 store holding the widened
rows, or of a dense store of the same type, and every comparison is strict: labels and distance bits at every rank
(compare_exact) or the bytes of the output, exact ties on (the handles' default)."""
import numpy as np
import pytest

from gamma_amd import api
from oracle import binding as B
from tests import fixtures
from tests import sq8_ref as S
from tests.parity import compare_exact
from tests.test_gpu_group import WIDE, _same_lists
from tests.test_gpu_group_rawshard import _rows_once
from tests.test_gpu_rawf16 import rounded
from tests.test_gpu_rawi8 import ints

pytestmark = pytest.mark.gpu

DTYPES = ["float16", "uint8", "int8", "sq8"]
ESIZE = {"float16": 2, "uint8": 1, "int8": 1, "sq8": 1}
METRICS = [api.METRIC_L2, api.METRIC_IP]
# what each store says to a row it cannot hold (gamma_hip_store.cpp), and a value it cannot hold
REFUSAL = {"float16": (1e6, "outside binary16's range"), "uint8": (0.5, "not exactly storable"),
           "int8": (200.0, "not exactly storable"), "sq8": (float("nan"), "is not finite")}
NARROW_NAME = {"float16": "holds float16 rows", "uint8": "holds 8-bit rows", "int8": "holds 8-bit rows",
               "sq8": "holds scalar-quantised sq8 rows"}


def _rows(dtype, n, d, seed):
    """fp32 rows every value of which the store of this type takes: whole-range integers for the byte stores, Gaussians that
    binary16 rounds for float16, Gaussians of several scales for sq8"""
    if dtype in ("uint8", "int8"):
        return ints(n, d, dtype, seed)
    if dtype == "float16":
        return (3.0 * np.random.default_rng(seed).standard_normal((n, d))).astype(np.float32)
    return S.rows(n, d, seed)


def _ranges(x):
    """sq8 ranges from the first half of the rows: the other half clips"""
    h = x[:max(1, len(x) // 2)]
    return h.min(axis=0), h.max(axis=0)


def _widen(dtype, x, ranges=None):
    """the fp32 rows a store of this type holds for x"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if dtype == "float16":
        return rounded(x)
    if dtype == "sq8":
        return S.stored(x, *ranges)
    return x.copy()            # the byte stores are lossless


def _store(d, dtype, ranges=None, switch=True, nlist=4, M=4):
    """a handle with an (untrained) IVFPQ model of dimension d -- the shard entries ask for one -- and an empty raw store"""
    g = api.GammaHip(0)
    g.ivfpq_init(d, nlist, M, 8, api.METRIC_L2)
    g.raw_init(d, dtype)
    if dtype == "sq8" and ranges is not None:
        g.raw_sq8_set_ranges(*ranges)
    if switch and dtype != "float32":
        g.set_sparse_narrow_rows(True)
    return g


def _exact(g, q, nv, metric):
    """gamma_hip_ivfpq_shard_exact of vector ids 0 .. nv - 1 for every query"""
    import torch
    nq = len(q)
    tq = torch.from_numpy(np.ascontiguousarray(q)).cuda()
    ids = torch.arange(nv, dtype=torch.int64).repeat(nq, 1).contiguous().cuda()
    out = torch.empty((nq, nv), dtype=torch.float32, device="cuda")
    a = api.SearchArgs(metric=metric, nprobe=4, recall_num=nv, has_rank=True, **WIDE)
    g.ivfpq_shard_exact(tq.data_ptr(), nq, ids.data_ptr(), nv, a, out.data_ptr())
    g.synchronize()
    return out.cpu().numpy()


def test_the_switch_is_exported_and_off_on_a_fresh_handle():
    assert hasattr(api._lib.load(), "gamma_hip_set_sparse_narrow_rows")
    for dtype in DTYPES:
        x = _rows(dtype, 4, 8, 1)
        g = _store(8, dtype, _ranges(x), switch=False)
        try:
            for call in (lambda: g.raw_put(np.array([0], np.int64), x[:1]), lambda: g.raw_put(np.zeros(0, np.int64), x[:0]),
                         lambda: g.raw_drop(np.array([0], np.int64))):
                with pytest.raises(api.GammaHipError, match=NARROW_NAME[dtype]):
                    call()
            with pytest.raises(api.GammaHipError, match="reads fp32 rows and is not supported"):
                _exact(g, x[:1], 4, api.METRIC_L2)
            g.set_sparse_narrow_rows(True)
            g.raw_put(np.array([2], np.int64), x[:1])
            assert g.raw_sparse_stats() == dict(live=1, slots=1, free=0)
            g.set_sparse_narrow_rows(False)            # off again: refused again, the rows stay
            with pytest.raises(api.GammaHipError, match=NARROW_NAME[dtype]):
                g.raw_put(np.array([3], np.int64), x[:1])
            with pytest.raises(api.GammaHipError, match=NARROW_NAME[dtype]):
                g.raw_drop(np.array([2], np.int64))
            assert g.raw_sparse_stats() == dict(live=1, slots=1, free=0)
        finally:
            g.close()


@pytest.mark.parametrize("d", [20, 128])
@pytest.mark.parametrize("dtype", DTYPES)
def test_sparse_narrow_store_rewrites_drops_reuses_grows_and_clears(dtype, d, monkeypatch):
    """The script of test_sparse_store_rewrites_drops_reuses_and_clears (tests/test_gpu_group_rawshard.py) over a narrow store:
    raw_sparse_stats after every step, contents through _shard_exact (L2 and inner product) bit-identical to a dense store of
    the same type holding the same rows AND to a dense fp32 store holding the widened rows; vectors not held: the sentinel.
    d = 20: element loads (no multiple of 8), over a store that reallocates when it grows -- the last puts take it past its
    first capacity; d = 128: 16-byte loads, over a store that maps memory behind its rows where the runtime offers that."""
    if d == 20:
        monkeypatch.setenv("GAMMA_HIP_NO_RAW_VMM", "1")      # capacity max(rows needed, 1.5 x capacity, 1024) rows
    base = _rows(dtype, 3000, d, 11 + d)
    rg = _ranges(base) if dtype == "sq8" else None
    q = _rows(dtype, 8, d, 5)
    sp, dn, f32 = _store(d, dtype, rg), _store(d, dtype, rg), _store(d, "float32")
    nv = 64
    held = {}                       # vid -> row of `base` the sparse store should hold for it
    try:
        def put(vids, rows):
            sp.raw_put(np.asarray(vids, np.int64), base[np.asarray(rows)])
            for v, r in zip(vids, rows):
                held[int(v)] = int(r)

        def drop(vids):
            sp.raw_drop(np.asarray(vids, np.int64))
            for v in vids:
                held.pop(int(v), None)

        def check(slots, free):
            st = sp.raw_sparse_stats()
            assert st == dict(live=len(held), slots=slots, free=free), st
            assert sp.raw_count() == len(held) and sp.raw_elem_bytes() == ESIZE[dtype]
            mirror = np.zeros((nv, d), np.float32)           # row v = what the sparse store should hold for vid v
            if dtype == "sq8":
                mirror[:] = base[0]                          # (any storable row: the rows not held are not compared)
            for v, r in held.items():
                if v < nv:
                    mirror[v] = base[r]
            dn.raw_clear()
            dn.raw_append(mirror)
            f32.raw_clear()
            f32.raw_append(_widen(dtype, mirror, rg))
            have = np.zeros(nv, bool)
            have[[v for v in held if v < nv]] = True
            for metric in METRICS:
                e_sp, e_dn, e_32 = _exact(sp, q, nv, metric), _exact(dn, q, nv, metric), _exact(f32, q, nv, metric)
                sentinel = np.inf if metric == api.METRIC_L2 else -np.inf
                assert (e_sp[:, ~have] == sentinel).all()
                assert np.isfinite(e_sp[:, have]).all()
                assert e_sp[:, have].tobytes() == e_dn[:, have].tobytes()
                assert e_sp[:, have].tobytes() == e_32[:, have].tobytes()

        put([5, 9, 40], [100, 101, 102])
        check(3, 0)
        put([9], [200])                              # held: rewritten in place
        check(3, 0)
        put([9, 5, 9], [201, 202, 203])              # named twice in one call: the last one wins, still in place
        check(3, 0)
        drop([5, 63, 7777777])                       # 63 / 7777777: never held, ignored
        check(3, 1)
        put([7], [300])                              # the freed row is reused before the store grows
        check(3, 0)
        drop([7, 9])
        put([11, 12, 13], [301, 302, 303])           # two reused, one new
        check(4, 0)
        put([40, 20, 21], [400, 401, 402])           # in place + growth in one call
        check(6, 0)
        drop([40, 40])
        check(6, 1)
        # growth past the store's first capacity, in order and with a rewrite in the batch
        cap = sp.raw_stats()["capacity"]
        n = (cap if d == 20 else 1024) + 37
        assert d != 20 or (cap == 1024 and not sp.raw_stats()["in_place"])
        vids = 1000 + np.arange(n)
        put(list(vids), list(np.arange(n) % len(base)))
        check(6 + n - 1, 0)                          # (one freed row reused)
        assert d != 20 or sp.raw_stats()["capacity"] > cap
        put([3, 1000, 4], [500, 501, 502])
        check(6 + n - 1 + 2, 0)
        # dense entries refuse the sparse store, whatever the switch says
        for call in (lambda: sp.raw_gets(np.array([0], np.int64)), lambda: sp.raw_append(base[:1]),
                     lambda: sp.raw_write(0, base[:1])):
            with pytest.raises(api.GammaHipError, match="this shard's rows only"):
                call()
        sp.raw_clear()
        assert sp.raw_sparse_stats() == dict(live=0, slots=0, free=0) and sp.raw_elem_bytes() == ESIZE[dtype]
        held.clear()
        put([2], [7])                                # sparse again after the clear, same element type
        check(1, 0)
    finally:
        for g in (sp, dn, f32):
            g.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_refused_row_changes_nothing(dtype):
    d = 24
    base = _rows(dtype, 200, d, 3)
    rg = _ranges(base) if dtype == "sq8" else None
    bad_value, message = REFUSAL[dtype]
    g = _store(d, dtype, rg)
    try:
        g.raw_put(np.array([1, 2, 3, 30], np.int64), base[:4])
        g.raw_drop(np.array([2], np.int64))
        stats = g.raw_sparse_stats()
        before = [_exact(g, base[:4], 40, m).tobytes() for m in METRICS]
        rows = base[10:14].copy()
        rows[2, 5] = bad_value                       # the third row of the put
        # (held, freed-row and new vids in one call: none of them may be touched)
        with pytest.raises(api.GammaHipError, match=message):
            g.raw_put(np.array([1, 7, 8, 9], np.int64), rows)
        assert g.raw_sparse_stats() == stats == dict(live=3, slots=4, free=1)
        assert [_exact(g, base[:4], 40, m).tobytes() for m in METRICS] == before
        g.raw_put(np.array([1, 7], np.int64), rows[:2])      # the handle goes on
        assert g.raw_sparse_stats() == dict(live=4, slots=4, free=0)
    finally:
        g.close()


def test_an_sq8_put_needs_its_ranges_first():
    d = 16
    base = _rows("sq8", 50, d, 2)
    g = _store(d, "sq8", None)
    try:
        g.raw_put(np.zeros(0, np.int64), base[:0])           # the empty put that makes the store sparse asks for none
        with pytest.raises(api.GammaHipError, match="no ranges yet"):
            g.raw_put(np.array([0], np.int64), base[:1])
        assert g.raw_sparse_stats() == dict(live=0, slots=0, free=0)
        # the ranges of a store in its sparse form are fixed (a group compares its members' once, at set_raw_placement)
        with pytest.raises(api.GammaHipError, match="sparse form"):
            g.raw_sq8_set_ranges(*_ranges(base))
        g.raw_clear()
        g.raw_sq8_set_ranges(*_ranges(base))
        g.raw_put(np.array([0], np.int64), base[:1])
        assert g.raw_sparse_stats() == dict(live=1, slots=1, free=0)
    finally:
        g.close()


@pytest.mark.parametrize("d", [20, 128])
@pytest.mark.parametrize("dtype", DTYPES)
def test_export_exact_equals_the_fp32_store_of_the_widened_rows(dtype, d):
    """gamma_hip_ivfpq_shard_export_exact over a sparse narrow store: exported rows of 0, 1, 255, 256 and 300 entries (a partial
    and a second 256-chunk), each with a finite bound, a NaN bound (every entry) and a bound that admits nothing; ids the store
    does not hold, negative ids, ids beyond the table and entries carrying the sentinel are among them.  The output is
    byte-identical -- NaN payloads included -- to that of the fp32 sparse store holding the widened rows."""
    import torch
    rng = np.random.default_rng(17 + d)
    nvid, P, stride = 500, 4, 300
    base = _rows(dtype, nvid, d, 23 + d)
    rg = _ranges(base) if dtype == "sq8" else None
    held = np.sort(rng.choice(nvid, size=nvid * 2 // 3, replace=False)).astype(np.int64)
    nr, f32 = _store(d, dtype, rg), _store(d, "float32")
    try:
        order = rng.permutation(len(held))                   # (arrival order != vid order: slots are not the identity)
        nr.raw_put(held[order], base[held[order]])
        f32.raw_put(held, _widen(dtype, base[held], rg))
        lens = [0, 1, 255, 256, 300]
        nf = len(lens) * 3
        for metric in METRICS:
            l2 = metric == api.METRIC_L2
            sentinel = np.float32(np.inf if l2 else -np.inf)
            vals = rng.standard_normal((nf, stride)).astype(np.float32)
            ids = rng.integers(0, nvid, size=(nf, stride)).astype(np.int64)
            ids[:, 3::17] = -1                               # empty entries
            ids[:, 5::19] = nvid + 70000                     # beyond the vid -> row table
            vals[:, 7::13] = sentinel                        # filtered entries carry the sentinel
            off = np.zeros((nf, P + 1), np.int32)
            bound = np.zeros(nf, np.float32)
            for f in range(nf):
                n = lens[f % len(lens)]
                off[f] = np.minimum(np.arange(P + 1) * ((n + P - 1) // P), n)
                off[f, P] = n
                kind = f // len(lens)
                bound[f] = (0.3 if l2 else -0.3) if kind == 0 else np.nan if kind == 1 else (-1e30 if l2 else 1e30)
            xf = _rows(dtype, nf, d, 31)
            a = api.SearchArgs(metric=metric, nprobe=P, recall_num=100, has_rank=True, **WIDE)
            outs = []
            for g in (nr, f32):
                t = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (xf, vals, ids, off, bound)]
                ex = torch.full((nf, stride), 7.0, dtype=torch.float32, device="cuda")
                g.ivfpq_shard_export_exact(nf, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), stride,
                                           t[4].data_ptr(), a, ex.data_ptr())
                g.synchronize()
                outs.append(ex.cpu().numpy())
            assert outs[0].tobytes() == outs[1].tobytes()
            e = outs[0]
            is_held = np.isin(ids, held)
            for f in range(nf):
                n, kind = lens[f % len(lens)], f // len(lens)
                assert (e[f, n:] == 7.0).all()               # nothing beyond the row's entries is written
                inb = np.ones(n, bool) if kind == 1 else np.zeros(n, bool) if kind == 2 else \
                    (vals[f, :n] <= bound[f] if l2 else vals[f, :n] >= bound[f])
                want = inb & is_held[f, :n] & np.isfinite(vals[f, :n])
                assert np.isfinite(e[f, :n][want]).all()
                assert (e[f, :n][~want].view(np.uint32) == 0x7fc00000).all()     # the qNaN pattern, exactly
            assert np.isfinite(e).sum() > 200
    finally:
        nr.close()
        f32.close()


# ---- the group ----------------------------------------------------------------------------------------------------------------
NDUP = 200


@pytest.fixture(scope="module")
def case():
    return fixtures.trained_case(d=32, nlist=64, M=8, N=20000, nq=64, metric=B.METRIC_L2)


_typed = {}


def _typed_case(case, dtype):
    """The fixture's vectors as a store of this type takes them, NDUP of them duplicated (exact ties: the tie phase runs), and
    the trained state moved along: uint8 takes the SIFT-like integers as they are; int8 takes them shifted by -128 (the coarse
    centroids shift too, the residuals and their codebooks stay); float16 and sq8 take them scaled by 0.37 (centroids and
    codebooks scale too), so that binary16 rounds them and the sq8 codes quantise them.  Built once per type, left unchanged."""
    if dtype in _typed:
        return _typed[dtype]
    base, q, cc, pq = case["base"].copy(), case["q"].copy(), case["cc"], case["pq"]
    rng = np.random.default_rng(77)
    dup = rng.choice(len(base), size=2 * NDUP, replace=False)
    base[dup[NDUP:]] = base[dup[:NDUP]]
    q = np.concatenate([base[dup[:24]], q]).astype(np.float32)       # queries at duplicated vectors: ties inside the top k
    if dtype == "int8":
        base, q, cc = base - 128.0, q - 128.0, cc - np.float32(128.0)
    elif dtype in ("float16", "sq8"):
        s = np.float32(0.37)
        base, q, cc, pq = base * s, q * s, cc * s, pq * s
    c = dict(case, base=np.ascontiguousarray(base, np.float32), q=np.ascontiguousarray(q, np.float32),
             cc=np.ascontiguousarray(cc, np.float32), pq=np.ascontiguousarray(pq, np.float32), dtype=dtype, oracle=None)
    c["ranges"] = _ranges(c["base"][:6000]) if dtype == "sq8" else None
    c["wide"] = _widen(dtype, c["base"], c["ranges"])
    _typed[dtype] = c
    return c


def _member_init(m, c, dtype=None, switch=True):
    dtype = dtype or c["dtype"]
    m.ivfpq_init(c["d"], c["nlist"], c["M"], 8, api.METRIC_L2, 1000)
    m.ivfpq_set_trained(c["cc"], c["pq"], None)
    m.raw_init(c["d"], dtype)
    if dtype == "sq8":
        m.raw_sq8_set_ranges(*c["ranges"])
    if switch:
        m.set_sparse_narrow_rows(True)


def _narrow_group(c, W):
    grp = api.GammaHipGroup([0] * W)
    for m in grp.members:
        _member_init(m, c)
    grp.set_raw_placement(True)
    assert grp.raw_placement()
    grp.set_owners(np.random.default_rng(W).integers(1, 100, size=c["nlist"]))      # uneven owner weights
    return grp


def _dense_single(c):
    """ONE handle holding every list, with a dense store of the same type"""
    g = api.GammaHip(0)
    _member_init(g, c, switch=False)
    return g


SEARCHES = ((api.METRIC_L2, True, 8, 100, 10), (api.METRIC_IP, True, 16, 64, 5), (api.METRIC_L2, False, 12, 50, 10),
            (api.METRIC_IP, False, 8, 40, 10))


def _compare(c, one, grp, nq=None):
    q = c["q"][:nq] if nq else c["q"]
    res = []
    for metric, has_rank, P, R, k in SEARCHES:
        a = api.SearchArgs(metric=metric, nprobe=P, recall_num=R, has_rank=has_rank, **WIDE)
        D, I = one.ivfpq_search(q, k, a)
        Dg, Ig = grp.ivfpq_search(q, k, a)
        compare_exact(D, I, Dg, Ig)
        res.append((Dg.tobytes(), Ig.tobytes()))
    return res


@pytest.mark.parametrize("W", [2, 3])
@pytest.mark.parametrize("dtype", DTYPES)
def test_narrow_rawshard_group_is_the_single_handle_of_the_same_type(case, dtype, W):
    """Add in batches, Update 300 vectors (some change member), Delete, compact: after every step the group's searches with
    has_rank 1 and 0, L2 and inner product, equal those of ONE handle with a dense store of the same type; the tie phase runs
    (so the typed export runs); every row lives exactly once in 2 or 1 bytes per element; a group add with an unstorable row
    changes nothing anywhere.  W = 2 is also held against the oracle over the widened rows."""
    c = _typed_case(case, dtype)
    base, N, d = c["base"], len(c["base"]), c["d"]
    one, grp = _dense_single(c), _narrow_group(c, W)
    try:
        for m in grp.members:
            m.tie_stats(reset=True)
        for i0 in range(0, N, 5000):
            one.raw_append(base[i0:i0 + 5000])
            one.add(base[i0:i0 + 5000], i0)
            grp.add(base[i0:i0 + 5000], i0)
            _compare(c, one, grp, nq=None if i0 + 5000 >= N else 30)
        _same_lists(c, grp, one)
        stats, owners = _rows_once(c, grp, N)
        for i, m in enumerate(grp.members):
            assert m.raw_elem_bytes() == ESIZE[dtype]
            assert stats[i]["live"] == sum(m.list_size(l) for l in range(c["nlist"]) if owners[l] == i) and stats[i]["live"] > 0
        # the tie phase of a has_rank search runs (flagged queries > 0): the exact distances of its exported streams come from
        # the typed export kernel
        for metric, has_rank, P, R, k in SEARCHES[:2]:
            for m in grp.members:
                m.tie_stats(reset=True)
            grp.ivfpq_search(c["q"], k, api.SearchArgs(metric=metric, nprobe=P, recall_num=R, has_rank=has_rank, **WIDE))
            ts = [m.tie_stats() for m in grp.members]
            flagged = sum(t["replayed"] + t["cut_ties"] for t in ts)
            print("narrow rawshard %s W=%d metric=%d: %d queries flagged (cut ties + replays) %s" % (dtype, W, metric, flagged, ts))
            assert flagged > 0 and sum(t["replayed"] for t in ts) > 0
        if W == 2:                                           # the oracle over the widened rows, same lists
            o = B.OracleIVFPQ(d, c["nlist"], c["M"], 8, B.METRIC_L2, bucket_init_size=1000)
            o.set_trained(c["cc"], c["pq"], None)
            B.lib().go_set_assign_mode(0)
            assert o.add(base)
            o.set_raw(c["wide"])
            for metric, has_rank, P, R, k in (SEARCHES[0], SEARCHES[2]):
                D, I = o.search(c["q"], k, P, recall_num=R, has_rank=has_rank, metric=metric, ctx=B.make_ctx(**WIDE))
                Dg, Ig = grp.ivfpq_search(c["q"], k, api.SearchArgs(metric=metric, nprobe=P, recall_num=R, has_rank=has_rank, **WIDE))
                compare_exact(D, I, Dg, Ig)

        # a group add with one unstorable row: refused with the store's message, nothing changed on any member
        def state():
            return ([m.raw_sparse_stats() for m in grp.members], [grp.list_size(l) for l in range(c["nlist"])])
        before, res = state(), _compare(c, one, grp, nq=20)
        rows = base[:50].copy()
        rows[31, 7] = REFUSAL[dtype][0]
        with pytest.raises(api.GammaHipError, match=REFUSAL[dtype][1]):
            grp.add(rows, N)
        with pytest.raises(api.GammaHipError, match=REFUSAL[dtype][1]):
            grp.update(np.arange(50, dtype=np.int64), rows)
        with pytest.raises(api.GammaHipError, match=REFUSAL[dtype][1]):
            grp.raw_put(np.arange(50, dtype=np.int64), rows)
        assert state() == before and _compare(c, one, grp, nq=20) == res

        # Update: 300 vectors, 150 of them replaced by a vector that lives on another member; five vids named twice
        lno = np.asarray(one.encode(base)[0])
        own_of = owners[lno]
        rng = np.random.default_rng(21 + W)
        vids = rng.choice(N, size=300, replace=False).astype(np.int64)
        src = np.array([rng.choice(np.nonzero(own_of != own_of[v])[0]) if i < 150 else rng.integers(0, N)
                        for i, v in enumerate(vids)])
        b_vids = np.concatenate([vids[:5], vids])
        vecs = np.concatenate([base[rng.integers(0, N, size=5)], base[src]])
        held0 = np.concatenate([m.has_vid(np.arange(N, dtype=np.int64))[None] for m in grp.members])
        one.update_batch(b_vids, vecs)
        one.raw_update_batch(b_vids, vecs)
        grp.update(b_vids, vecs)
        _same_lists(c, grp, one)
        stats2, _ = _rows_once(c, grp, N)
        held = np.concatenate([m.has_vid(np.arange(N, dtype=np.int64))[None] for m in grp.members])
        assert (held.sum(axis=0) == 1).all()
        assert (held0 != held).any(axis=0).sum() >= 100                      # vectors changed member, their rows with them
        for i in range(W):
            assert stats2[i]["live"] == int(held[i].sum())
        _compare(c, one, grp)
        # Delete, then compaction
        dead = rng.choice(N, size=N // 3, replace=False).astype(np.int64)
        bm = np.zeros(N // 8 + 1, np.uint8)
        np.bitwise_or.at(bm, dead >> 3, (1 << (dead & 7)).astype(np.uint8))
        one.bitmap_upload(bm, N)
        one.delete(dead)
        grp.each(lambda m: m.bitmap_upload(bm, N))
        grp.delete(dead)
        _compare(c, one, grp)
        one.compact_if_need()
        grp.compact_if_need()
        _compare(c, one, grp)
        _rows_once(c, grp, N)
        for m in grp.members:
            assert m.raw_elem_bytes() == ESIZE[dtype]
    finally:
        one.close()
        grp.close()


def test_members_of_mixed_element_types_or_with_the_switch_off_are_refused(case):
    c = _typed_case(case, "uint8")
    for kinds, switch, message in ((("uint8", "int8"), True, "differ in element type"),
                                   (("uint8", "float32"), True, "differ in element type"),
                                   (("uint8", "uint8"), False, NARROW_NAME["uint8"])):     # switch off: as before
        grp = api.GammaHipGroup([0, 0])
        try:
            for m, dtype in zip(grp.members, kinds):
                _member_init(m, c, dtype, switch=switch and dtype != "float32")
            with pytest.raises(api.GammaHipError, match=message):
                grp.set_raw_placement(True)
            assert not grp.raw_placement()
        finally:
            grp.close()
    # sq8 members decoding through different ranges
    c = _typed_case(case, "sq8")
    grp = api.GammaHipGroup([0, 0])
    try:
        for m in grp.members:
            _member_init(m, c)
        grp.members[1].raw_clear()
        lo, hi = c["ranges"]
        grp.members[1].raw_sq8_set_ranges(lo, hi + 1.0)
        with pytest.raises(api.GammaHipError, match="sq8 ranges"):
            grp.set_raw_placement(True)
    finally:
        grp.close()
