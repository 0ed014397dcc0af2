"""GPU: raw vectors sharded with their lists in the in-process group (gamma_hip_group_set_raw_placement, the sparse raw
store's rewrite / drop / clear, the plugins' "raw_placement" key).  Every member lives on device 0, as in
tests/test_gpu_group.py, whose builders and yardstick this file reuses: the single handle holding every list and every row.
Every comparison is strict -- labels equal and distance bits equal at every rank (compare_exact), no tolerance."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from gamma_amd import api, synth
from oracle import binding as B
from tests import fixtures
from tests.parity import compare_exact
from tests.test_gpu_group import WIDE, _group, _same_lists, _single

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def case():
    return fixtures.trained_case(d=32, nlist=64, M=8, N=20000, nq=64, metric=B.METRIC_L2)


def _rawshard_group(case, W, weights=None, add=True):
    grp = api.GammaHipGroup([0] * W)
    for m in grp.members:
        m.ivfpq_init(case["d"], case["nlist"], case["M"], 8, api.METRIC_L2, 1000)
        m.ivfpq_set_trained(case["cc"], case["pq"], None)
        m.raw_init(case["d"])
    grp.set_raw_placement(True)
    assert grp.raw_placement()
    grp.set_owners(weights)
    if add:
        for i0 in range(0, len(case["base"]), 5000):
            grp.add(case["base"][i0:i0 + 5000], i0)
    return grp


def _rows_once(case, grp, n_live):
    """every row exactly once, at the owner of its vector's list"""
    W = len(grp.members)
    owners = np.array([grp.owner(l) for l in range(case["nlist"])])
    stats = [m.raw_sparse_stats() for m in grp.members]
    assert sum(s["live"] for s in stats) == n_live, stats
    for i, m in enumerate(grp.members):
        # (a list's size counts superseded entries too: the callers pass groups without them, or compare live counts)
        assert m.raw_count() == stats[i]["live"]
        assert stats[i]["live"] + stats[i]["free"] == stats[i]["slots"], stats[i]
    return stats, owners


def test_new_abi_entries_are_exported():
    L = api._lib.load()
    for n in ("gamma_hip_raw_drop", "gamma_hip_raw_clear", "gamma_hip_raw_sparse_stats", "gamma_hip_group_set_raw_placement",
              "gamma_hip_group_raw_placement", "gamma_hip_group_raw_put"):
        assert hasattr(L, n), n


def test_sparse_store_rewrites_drops_reuses_and_clears(case):
    """The store by itself: a put of a held vid rewrites its row in place (the slot count stays), dropped rows go to a free
    list that later puts reuse before the store grows, unknown vids are ignored, a dense store refuses a drop, clear gives the
    state after raw_init back.  Row CONTENTS are read through gamma_hip_ivfpq_shard_exact and compared with a dense store's
    answer for the same vectors (bit for bit)."""
    import torch
    d, base = case["d"], case["base"]
    sp, dn = api.GammaHip(0), api.GammaHip(0)
    try:
        for g in (sp, dn):
            g.ivfpq_init(d, case["nlist"], case["M"], 8, api.METRIC_L2, 1000)
            g.ivfpq_set_trained(case["cc"], case["pq"], None)
            g.raw_init(d)
        held = {}                       # vid -> row of `base` the sparse store should hold for it

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
            assert sp.raw_count() == len(held)
            # a dense mirror with row v = what the sparse store should hold for vid v (zeros where it holds nothing)
            nv = 64
            mirror = np.zeros((nv, d), np.float32)
            for v, r in held.items():
                mirror[v] = base[r]
            dn.raw_clear()
            dn.raw_append(mirror)
            q = torch.from_numpy(case["q"][:8].copy()).cuda()
            ids = torch.arange(nv, dtype=torch.int64).repeat(8, 1).cuda()
            a = api.SearchArgs(metric=api.METRIC_L2, nprobe=4, recall_num=nv, has_rank=True, **WIDE)
            e_sp = torch.empty((8, nv), dtype=torch.float32, device="cuda")
            e_dn = torch.empty((8, nv), dtype=torch.float32, device="cuda")
            sp.ivfpq_shard_exact(q.data_ptr(), 8, ids.data_ptr(), nv, a, e_sp.data_ptr())
            dn.ivfpq_shard_exact(q.data_ptr(), 8, ids.data_ptr(), nv, a, e_dn.data_ptr())
            sp.synchronize()
            dn.synchronize()
            e_sp, e_dn = e_sp.cpu().numpy(), e_dn.cpu().numpy()
            have = np.zeros(nv, bool)
            have[list(held)] = True
            assert np.isinf(e_sp[:, ~have]).all()                                    # not held: the sentinel
            assert e_sp[:, have].tobytes() == e_dn[:, have].tobytes()

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
        # a dense store refuses; clear makes it an empty store that may become sparse, and back
        with pytest.raises(api.GammaHipError):
            dn.raw_drop(np.array([1], np.int64))
        dn.raw_clear()
        assert dn.raw_count() == 0 and dn.raw_stats()["rows"] == 0 and dn.raw_stats()["capacity"] == 0
        dn.raw_put(np.array([3], np.int64), base[:1])
        assert dn.raw_sparse_stats() == dict(live=1, slots=1, free=0)
        with pytest.raises(api.GammaHipError):
            dn.raw_append(base[:4])                  # sparse now
        dn.raw_clear()
        assert dn.raw_sparse_stats() == dict(live=0, slots=0, free=0)
        dn.raw_append(base[:4])
        assert dn.raw_count() == 4
    finally:
        sp.close()
        dn.close()


@pytest.fixture(scope="module")
def full(case):
    g = _single(case)
    yield g
    g.close()


@pytest.mark.parametrize("W,weights", [(1, None), (2, "sizes"), (2, None), (3, None), (3, "sizes")])
def test_rawshard_group_is_the_replicated_group_is_the_single_handle(case, full, W, weights):
    """Sharded-raw group == replicated-raw group == single handle: L2 and inner product, has_rank 1 and 0, a score window, a
    range filter, deleted docs, batches below and above the 20 queries of the coarse-mode rule, both owner weightings."""
    base, N = case["base"], len(case["base"])
    sizes = np.array([full.list_size(l) for l in range(case["nlist"])], dtype=np.int64)
    w = sizes if weights == "sizes" else None
    shd, rep = _rawshard_group(case, W, w), _group(case, W, w)
    one = _single(case)            # (its own single handle: the deletes below change it)
    try:
        _same_lists(case, shd, one)
        stats, owners = _rows_once(case, shd, N)
        for i in range(W):
            assert stats[i]["live"] == sizes[owners == i].sum() and stats[i]["free"] == 0

        def check(extra=None, nqs=(1, 7, 19, 20, 64, 700)):
            for nq in nqs:
                q = synth.sift_like(nq, d=case["d"], seed=277 + nq)
                for metric, has_rank, P, R, k in ((api.METRIC_L2, True, 8, 100, 10), (api.METRIC_IP, True, 16, 64, 5),
                                                  (api.METRIC_L2, False, 12, 50, 10), (api.METRIC_IP, False, 8, 40, 10),
                                                  (api.METRIC_L2, True, 64, 200, 20)):
                    kw = dict(WIDE)
                    kw.update(extra(metric, q, P, R, k) if extra else {})
                    a = api.SearchArgs(metric=metric, nprobe=P, recall_num=R, has_rank=has_rank, **kw)
                    D, I = one.ivfpq_search(q, k, a)
                    Dr, Ir = rep.ivfpq_search(q, k, a)
                    Ds, Is = shd.ivfpq_search(q, k, a)
                    compare_exact(D, I, Dr, Ir)
                    compare_exact(D, I, Ds, Is)
        check()

        # a score window that cuts into the results: from the median exact distance of the single handle's answers
        def window(metric, q, P, R, k):
            a = api.SearchArgs(metric=metric, nprobe=P, recall_num=R, has_rank=True, **WIDE)
            D, I = one.ivfpq_search(q, k, a)
            mid = float(np.median(D[I >= 0]))
            return dict(min_score=-3e38, max_score=mid) if metric == api.METRIC_L2 else dict(min_score=mid, max_score=3e38)
        check(window, nqs=(7, 64))
        # a request's range filter
        allowed = np.nonzero(np.random.default_rng(5).random(N) < 0.3)[0]
        check(lambda *_: dict(range_filters=[api.make_range_filter(allowed)]), nqs=(5, 40))
        # deleted docs
        dead = np.random.default_rng(6).choice(N, size=N // 3, replace=False).astype(np.int64)
        bm = np.zeros(N // 8 + 1, np.uint8)
        np.bitwise_or.at(bm, dead >> 3, (1 << (dead & 7)).astype(np.uint8))
        one.bitmap_upload(bm, N)
        one.delete(dead)
        for g in (shd, rep):
            g.each(lambda m: m.bitmap_upload(bm, N))
            g.delete(dead)
        check(nqs=(7, 64))
        q = synth.sift_like(64, d=case["d"], seed=8)
        Ds, Is = shd.ivfpq_search(q, 10, api.SearchArgs(metric=api.METRIC_L2, nprobe=16, recall_num=100, has_rank=True, **WIDE))
        assert not np.isin(Is, dead).any()
    finally:
        for g in (shd, rep, one):
            g.close()


def test_placement_switch_rules(case):
    """Only while no member holds a row; never with replicated lists; group raw_put only in sharded mode."""
    grp = api.GammaHipGroup([0, 0])
    try:
        for m in grp.members:
            m.ivfpq_init(case["d"], case["nlist"], case["M"], 8, api.METRIC_L2, 1000)
            m.ivfpq_set_trained(case["cc"], case["pq"], None)
            m.raw_init(case["d"])
        assert not grp.raw_placement()
        with pytest.raises(api.GammaHipError):
            grp.raw_put(np.array([0], np.int64), case["base"][:1])
        grp.members[1].raw_append(case["base"][:10])
        with pytest.raises(api.GammaHipError):
            grp.set_raw_placement(True)
        grp.members[1].raw_clear()
        grp.set_raw_placement(True)
        grp.set_raw_placement(False)                # no row yet: back to rows by vector id
        assert not grp.raw_placement()
        grp.members[0].raw_append(case["base"][:3])
        grp.members[0].raw_clear()
        grp.set_raw_placement(True)
        with pytest.raises(api.GammaHipError):
            grp.set_placement(True)
        grp.set_owners(None)
        grp.add(case["base"][:100], 0)
        with pytest.raises(api.GammaHipError):
            grp.set_raw_placement(False)            # rows are written
    finally:
        grp.close()
    grp = api.GammaHipGroup([0, 0])
    try:
        grp.set_placement(True)
        for m in grp.members:
            m.ivfpq_init(case["d"], case["nlist"], case["M"], 8, api.METRIC_L2, 1000)
            m.raw_init(case["d"])
        with pytest.raises(api.GammaHipError):
            grp.set_raw_placement(True)
    finally:
        grp.close()


@pytest.mark.parametrize("tag,W", [("l2", 2), ("ip", 3), ("l2", 1)])
def test_rawshard_group_keeps_the_reference_order_inside_ties(tag, W):
    """The tie goldens of test_sharded_group_keeps_the_reference_order_inside_ties with every row at its list's owner: keys
    through add_keys, rows through the group's raw_put.  The tie phase must run (flagged queries > 0) and the labels are the
    pinned oracle's, strictly."""
    from tests.test_oracle_golden import load_ties
    z, o, base, metric = load_ties(tag)
    d, nlist, M = int(z["d"]), int(z["nlist"]), int(z["M"])
    sizes = z["list_sizes_" + tag]
    offs = np.concatenate([[0], np.cumsum(sizes)])
    grp = api.GammaHipGroup([0] * W)
    try:
        for m in grp.members:
            m.ivfpq_init(d, nlist, M, 8, metric)
            m.ivfpq_set_trained(z["cc_" + tag], z["pq_" + tag], None)
            m.raw_init(d)
        grp.set_raw_placement(True)
        grp.set_owners(sizes)
        for l in range(nlist):
            if sizes[l]:
                grp.add_keys(l, z["list_ids_" + tag][offs[l]:offs[l + 1]], z["list_codes_" + tag][offs[l]:offs[l + 1]])
        vids = np.arange(len(base), dtype=np.int64)
        extra = np.array([len(base) + 7], np.int64)                     # a vid nobody lists
        for i0 in range(0, len(base), 3000):
            v = vids[i0:i0 + 3000]
            last = i0 + 3000 >= len(base)
            skipped = grp.raw_put(np.concatenate([v, extra]) if last else v, np.concatenate([base[v], base[:1]]) if last else base[v])
            assert skipped == (1 if last else 0)
        listed = np.concatenate([m.has_vid(vids)[None] for m in grp.members]).sum(axis=0)
        assert sum(m.raw_sparse_stats()["live"] for m in grp.members) == int((listed > 0).sum())
        ctx = B.make_ctx(**WIDE)
        for m in grp.members:
            m.tie_stats(reset=True)
        replayed_with_rank = 0
        for nprobe, R, k, has_rank in ((12, 60, 10, True), (6, 40, 10, False), (16, 100, 20, True)):
            D1, I1 = o.search(z["q"], k, nprobe, recall_num=R, has_rank=has_rank, metric=metric, ctx=ctx, coarse_mode=0)
            a = api.SearchArgs(metric=metric, nprobe=nprobe, recall_num=R, has_rank=has_rank, coarse_mode=0, **WIDE)
            for reps in (1, 15):
                q = np.tile(z["q"], (reps, 1))[:len(z["q"]) * reps - (reps > 1)]
                for m in grp.members:
                    m.tie_stats(reset=True)
                Dg, Ig = grp.ivfpq_search(q, k, a)
                flagged = sum(m.tie_stats()["replayed"] + m.tie_stats()["cut_ties"] for m in grp.members)
                print("ties %s W=%d nprobe=%d R=%d rank=%d nq=%d: %d queries flagged (cut ties + replays)" % (tag, W, nprobe, R, has_rank, len(q), flagged))
                replayed_with_rank += flagged if has_rank else 0
                compare_exact(np.tile(D1, (reps, 1))[:len(q)], np.tile(I1, (reps, 1))[:len(q)], Dg, Ig)
        assert replayed_with_rank > 0           # the tie phase ran with travelled exact distances
    finally:
        grp.close()


def test_each_row_exactly_once_and_memory(case, full):
    """After adding N vectors: live rows sum to N, each member holds the rows of its lists, dense entries refuse, and the
    group's memory in sharded mode is smaller than in replicated mode by at least (W - 1) N d 4 bytes minus W times the
    store's growth granularity -- which is read from the library: the rows a fresh store holding one row has room for."""
    W, N, d = 3, len(case["base"]), case["d"]
    probe = api.GammaHip(0)
    try:
        probe.raw_init(d)
        probe.raw_put(np.array([0], np.int64), case["base"][:1])
        gran = probe.raw_stats()["capacity"] * d * 4
    finally:
        probe.close()
    assert gran > 0
    shd, rep = _rawshard_group(case, W), _group(case, W)
    try:
        stats, owners = _rows_once(case, shd, N)
        for i, m in enumerate(shd.members):
            assert stats[i]["live"] == sum(full.list_size(l) for l in range(case["nlist"]) if owners[l] == i)
            assert stats[i]["live"] == sum(m.list_size(l) for l in range(case["nlist"]) if owners[l] == i)
            assert stats[i]["free"] == 0 and stats[i]["slots"] == stats[i]["live"]
            assert m.raw_count() == stats[i]["live"]
            assert m.raw_stats()["rows"] == stats[i]["slots"]
            for call in (lambda: m.raw_gets(np.array([0], np.int64)), lambda: m.raw_append(case["base"][:1]),
                         lambda: m.raw_write(0, case["base"][:1]), lambda: m.raw_update(0, case["base"][0])):
                with pytest.raises(api.GammaHipError):
                    call()
        held = np.concatenate([m.has_vid(np.arange(N, dtype=np.int64))[None] for m in shd.members])
        assert (held.sum(axis=0) == 1).all()
        ms, mr = shd.total_mem_bytes(), rep.total_mem_bytes()
        print("group memory, W=%d N=%d d=%d: replicated rows %d bytes, sharded rows %d bytes, granularity %d" % (W, N, d, mr, ms, gran))
        assert mr - ms >= (W - 1) * N * d * 4 - W * gran
        assert ms < mr or (W - 1) * N * d * 4 <= W * gran
    finally:
        shd.close()
        rep.close()


def test_updates_move_rows_with_their_vectors(case):
    """A batch that moves M vectors to lists of other members, then back, for several rounds, with a vid named twice in one
    batch: results equal the single handle given the same updates, live rows still sum to N, and the rows allocated over all
    members never exceed N + M -- freed rows are reused."""
    W, N, d, base = 3, len(case["base"]), case["d"], case["base"]
    one, shd = _single(case), _rawshard_group(case, W)
    try:
        owners = np.array([shd.owner(l) for l in range(case["nlist"])])
        lno = np.asarray(one.encode(base)[0])
        own_of = owners[lno]                                            # member that holds each vector now
        rng = np.random.default_rng(21)
        M = 300
        vids = rng.choice(N, size=M, replace=False).astype(np.int64)
        # for every chosen vid a replacement vector that lives on ANOTHER member
        away = np.array([rng.choice(np.nonzero(own_of != own_of[v])[0]) for v in vids])
        # the batch names five vids twice: first a vector of a third place, then the one that counts
        third = np.array([rng.choice(np.nonzero(own_of != own_of[v])[0]) for v in vids[:5]])
        b_vids = np.concatenate([vids[:5], vids])
        out_vecs = np.concatenate([base[third], base[away]])
        back_vecs = np.concatenate([base[third], base[vids]])
        a = api.SearchArgs(metric=api.METRIC_L2, nprobe=16, recall_num=100, has_rank=True, **WIDE)
        q = synth.sift_like(200, d=d, seed=9)
        cur = base.copy()
        for rnd in range(6):
            vecs = out_vecs if rnd % 2 == 0 else back_vecs
            one.update_batch(b_vids, vecs)
            for v, x in zip(b_vids, vecs):
                one.raw_update(int(v), x)
                cur[v] = x
            shd.update(b_vids, vecs)
            _same_lists(case, shd, one)
            stats, _ = _rows_once(case, shd, N)
            slots = sum(s["slots"] for s in stats)
            print("round %d: rows allocated %d (N = %d, M = %d), free %d" % (rnd, slots, N, M, sum(s["free"] for s in stats)))
            assert slots <= N + M
            # every vector's row is where its list entry is
            held = np.concatenate([m.has_vid(np.arange(N, dtype=np.int64))[None] for m in shd.members])
            assert (held.sum(axis=0) == 1).all()
            for i, m in enumerate(shd.members):
                assert stats[i]["live"] == int(held[i].sum())
            for nq in (7, 200):
                D, I = one.ivfpq_search(q[:nq], 10, a)
                Dg, Ig = shd.ivfpq_search(q[:nq], 10, a)
                compare_exact(D, I, Dg, Ig)
        # a put of held vids through the group: in place, nothing allocated
        before = [m.raw_sparse_stats() for m in shd.members]
        assert shd.raw_put(vids[:50], cur[vids[:50]]) == 0
        assert [m.raw_sparse_stats() for m in shd.members] == before
        # Delete + compaction leave the rows alone and the results equal
        dead = rng.choice(N, size=N // 3, replace=False).astype(np.int64)
        bm = np.zeros(N // 8 + 1, np.uint8)
        np.bitwise_or.at(bm, dead >> 3, (1 << (dead & 7)).astype(np.uint8))
        one.bitmap_upload(bm, N)
        one.delete(dead)
        one.compact_if_need()
        shd.each(lambda m: m.bitmap_upload(bm, N))
        shd.delete(dead)
        shd.compact_if_need()
        D, I = one.ivfpq_search(q, 10, a)
        Dg, Ig = shd.ivfpq_search(q, 10, a)
        compare_exact(D, I, Dg, Ig)
    finally:
        one.close()
        shd.close()


MODEL = '{"ncentroids": %d, "nsubvector": %d, "nprobe": 8, "metric_type": "L2"%s}'
SHARDED = ', "devices": "0,0,0", "raw_placement": "sharded"'


def test_plugin_raw_placement_key(case):
    """HIPIVFPQ with "devices": "0,0,0", "raw_placement": "sharded" == the one-GPU plugin through the whole script: brute
    force before training, Indexing, Add in several batches, Update, Delete, Search, Dump, Load into a fresh model, Search.
    Once the rows are sharded a brute_force_search request is refused (non-zero) and the model keeps serving; bad
    combinations are rejected at Init."""
    from gamma_amd import plugin
    base, q = case["base"], case["q"]
    mk = lambda extra: plugin.PluginModel("HIPIVFPQ", case["d"], MODEL % (case["nlist"], case["M"], extra), indexing_size=5000)
    ms = [mk(""), mk(SHARDED)]
    try:
        req = '{"metric_type": "L2", "recall_num": 100, "nprobe": 8}'
        for m in ms:
            m.store(base)
        D, I = ms[0].search(q, 10, req)                       # untrained: brute force (member 0's mirror in the sharded model)
        Dg, Ig = ms[1].search(q, 10, req)
        compare_exact(D, I, Dg, Ig)
        D, I = ms[0].search(q[:5], 10, req, brute_force=True)
        Dg, Ig = ms[1].search(q[:5], 10, req, brute_force=True)
        compare_exact(D, I, Dg, Ig)
        for m in ms:
            assert m.indexing() == 0
            for i0, i1 in ((0, 5000), (5000, 5019), (5019, 12000), (12000, len(base))):
                assert m.add(base[i0:i1])
        for n in (len(q), 5):
            for has_rank in (True, False):
                D, I = ms[0].search(q[:n], 10, req, has_rank=has_rank)
                Dg, Ig = ms[1].search(q[:n], 10, req, has_rank=has_rank)
                compare_exact(D, I, Dg, Ig)
        # no device holds every row now: never a silent wrong answer, and the model keeps serving
        with pytest.raises(api.GammaHipError):
            ms[1].search(q[:5], 10, req, brute_force=True)
        Dg, Ig = ms[1].search(q, 10, req)
        compare_exact(*ms[0].search(q, 10, req), Dg, Ig)
        rng = np.random.default_rng(2)
        vids = rng.choice(len(base), size=200, replace=False).astype(np.int64)
        vids = np.concatenate([vids, vids[:4]])
        vecs = base[rng.integers(0, len(base), size=len(vids))].copy()
        dead = rng.choice(len(base), size=2000, replace=False).astype(np.int64)
        b2 = base.copy()
        for v, x in zip(vids, vecs):
            b2[v] = x
        for m in ms:
            assert m.update_batch(vids, vecs) == 0
            assert m.delete(dead) == 0
        D, I = ms[0].search(q, 10, req)
        Dg, Ig = ms[1].search(q, 10, req)
        compare_exact(D, I, Dg, Ig)
        assert not np.isin(Ig, dead).any()
        assert ms[1].mem_bytes() > 0
        with tempfile.TemporaryDirectory() as td:
            assert ms[1].dump(td) == 0
            m2, m3 = mk(""), mk(SHARDED)
            try:
                for m in (m2, m3):
                    m.store(b2)
                    m.engine_bitmap_set(dead)
                    assert m.load(td) > 0
                    Dl, Il = m.search(q, 10, req)
                    compare_exact(D, I, Dl, Il)
                with pytest.raises(api.GammaHipError):
                    m3.search(q[:5], 10, req, brute_force=True)
                # the loaded model goes on: Add and Update after the Load
                more = synth.sift_like(300, d=case["d"], seed=91)
                b3 = np.concatenate([b2, more])
                for m in (m2, m3):
                    m.store(b3)
                    assert m.add(more)
                    assert m.update_batch(vids[:50], base[:50]) == 0
                compare_exact(*m2.search(q, 10, req), *m3.search(q, 10, req))
            finally:
                m2.close()
                m3.close()
    finally:
        for m in ms:
            m.close()
    for extra in (', "devices": "0,0", "placement": "replicate", "raw_placement": "sharded"',
                  ', "devices": "0", "raw_placement": "sharded"', ', "raw_placement": "sharded"',
                  ', "devices": "0,0", "raw_placement": "x"'):
        with pytest.raises(Exception):
            mk(extra)
    mk(', "devices": "0,0", "raw_placement": "replicated"').close()     # the default, spelled out


def _concurrent_body():
    """One writer thread updates through the plugin while two threads search the sharded model: every result is one of the
    two answers of the one-GPU plugin, before or after the batch."""
    import threading
    from gamma_amd import plugin
    case = fixtures.trained_case(d=32, nlist=64, M=8, N=20000, nq=64, metric=B.METRIC_L2)
    base, q = case["base"], case["q"]
    mk = lambda extra: plugin.PluginModel("HIPIVFPQ", case["d"], MODEL % (case["nlist"], case["M"], extra), indexing_size=5000)
    one, shd = mk(""), mk(SHARDED)
    try:
        for m in (one, shd):
            m.store(base)
            assert m.indexing() == 0
            for i0 in range(0, len(base), 5000):
                assert m.add(base[i0:i0 + 5000])
        req = '{"metric_type": "L2", "recall_num": 100, "nprobe": 16}'
        rng = np.random.default_rng(3)
        # the batch rewrites the queries' nearest neighbours, so that it changes the answers
        D0, I0 = one.search(q, 10, req)
        vids = np.unique(I0[:, :3][I0[:, :3] >= 0]).astype(np.int64)
        vecs = base[rng.integers(0, len(base), size=len(vids))].copy()
        assert one.update_batch(vids, vecs) == 0
        D1, I1 = one.search(q, 10, req)
        assert not np.array_equal(I0, I1)
        results, errors, done = [[], []], [], threading.Event()

        def searcher(t):
            try:
                while True:
                    last = done.is_set()
                    results[t].append(shd.search(q, 10, req))
                    if last:
                        return
            except Exception as e:          # noqa: BLE001
                errors.append(e)

        def writer():
            try:
                while min(len(r) for r in results) < 3 and not errors:
                    pass
                assert shd.update_batch(vids, vecs) == 0
            except Exception as e:          # noqa: BLE001
                errors.append(e)
            finally:
                done.set()

        th = [threading.Thread(target=searcher, args=(t,)) for t in range(2)] + [threading.Thread(target=writer)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errors, errors
        n_before = n_after = 0
        for r in results:
            for D, I in r:
                if np.array_equal(I, I0):
                    compare_exact(D0, I0, D, I)
                    n_before += 1
                else:
                    compare_exact(D1, I1, D, I)
                    n_after += 1
        compare_exact(D1, I1, *results[0][-1])
        compare_exact(D1, I1, *results[1][-1])
        assert n_before >= 3 and n_after >= 2
        print("concurrent ok: %d results before the batch, %d after" % (n_before, n_after))
    finally:
        one.close()
        shd.close()


def test_one_writer_two_searchers_through_the_plugin():
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c",
                        "from tests.test_gpu_group_rawshard import _concurrent_body; _concurrent_body()"],
                       cwd=ROOT, capture_output=True, text=True, timeout=330)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "concurrent ok" in r.stdout
