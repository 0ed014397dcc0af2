"""GPU: the IVFFLAT search of the in-process group (gamma_hip_group_ivfflat_search, include/gamma_hip.h).  Every member lives on
device 0; the yardstick is ONE handle fed the same calls, compared strictly -- labels equal and distance bits equal at every rank
(compare_exact); the one handle itself is held against the CPU oracle by tests/test_gpu_ivfflat*.py and, over the same shard
entries, by tests/test_gpu_ivfflat_shard.py.  Members are filled through the group's storage entries (gamma_hip_group_ivfpq_add / _update / _delete / _compact_if_need), which serve IVFFLAT members as they are."""
import numpy as np
import pytest

from gamma_amd import api
from oracle import binding as B
from tests import ivfflat_lm_data as LM
from tests import ivfflat_shard_ref as SR
from tests.parity import compare_exact

pytestmark = pytest.mark.gpu

L2, IP = B.METRIC_L2, B.METRIC_IP
WIDE = SR.WIDE
PLACEMENTS = ["replicated", "sharded", "replicate"]      # raw rows replicated | raw rows sharded | lists replicated


def _init(m, c):
    m.ivfflat_init(c.d, c.nlist, c.metric)
    m.ivfflat_set_trained(c.cc)
    m.raw_init(c.d)


def make_group(c, W, placement, by_size=False, rows=None, trained=None):
    """the case's rows added through the group in batches (the members assign them with their own coarse quantizer)"""
    rows = c.raw if rows is None else rows
    grp = api.GammaHipGroup([0] * W)
    for i, m in enumerate(grp.members):
        m.ivfflat_init(c.d, c.nlist, c.metric)
        if trained is None or trained[i]:
            m.ivfflat_set_trained(c.cc)
        m.raw_init(c.d)
    if placement == "replicate":
        grp.set_placement(True)
    if placement == "sharded":
        grp.set_raw_placement(True)
    weights = None
    if by_size:
        weights = np.bincount(B.ivfflat_assign(c.o, rows), minlength=c.nlist)
    grp.set_owners(weights)
    return grp


def fill(grp, placement, rows):
    for i0 in range(0, len(rows), 1000):
        grp.add(rows[i0:i0 + 1000], i0)
        if placement != "sharded":
            grp.each(lambda m: m.raw_append(rows[i0:i0 + 1000]))


def make_one(c, rows=None):
    rows = c.raw if rows is None else rows
    g = api.GammaHip(0)
    _init(g, c)
    for i0 in range(0, len(rows), 1000):
        g.add(rows[i0:i0 + 1000], i0)
        g.raw_append(rows[i0:i0 + 1000])
    return g


def check(grp, one, q, k, args):
    D1, I1 = one.ivfflat_search(q, k, args)
    D, I = grp.ivfflat_search(q, k, args)
    compare_exact(D1, I1, D, I)
    return D, I


@pytest.fixture(scope="module")
def plain():
    out = {}
    for metric in (L2, IP):
        c = LM.Case(128, "float32", metric, seed=80 + metric)
        out[metric] = (c, make_one(c))
    yield out
    for _, g in out.values():
        g.close()


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("by_size", [False, True], ids=["mod", "size"])
@pytest.mark.parametrize("W", [2, 3, 4])
@pytest.mark.parametrize("metric", [L2, IP], ids=["l2", "ip"])
def test_group_equals_one_handle(plain, metric, W, by_size, placement):
    c, one = plain[metric]
    grp = make_group(c, W, placement, by_size)
    try:
        fill(grp, placement, c.raw)
        args = api.SearchArgs(metric=metric, nprobe=4, exact_ties=1, **WIDE)
        rng = np.random.default_rng(W)
        big = (c.raw[rng.integers(0, c.N, 700)] + 0.5 * rng.standard_normal((700, c.d))).astype(np.float32)
        for nq in (1, 7, 64, 700):      # nq 1 leaves empty slices
            check(grp, one, big[:nq], 10, args)
        if placement == "sharded":
            st = [m.raw_sparse_stats()["live"] for m in grp.members]
            assert sum(st) == c.N and all(s < c.N for s in st)      # every row once, at the owner of its list
    finally:
        grp.close()


@pytest.mark.parametrize("placement", ["replicated", "sharded"])
def test_more_than_256_flagged_queries_run_two_rounds_of_the_tie_phase(placement):
    c = SR.TieCase(d=32, metric=L2, seed=3)
    one = make_one(c)
    grp = make_group(c, 2, placement)
    try:
        fill(grp, placement, c.raw)
        rng = np.random.default_rng(9)
        q = (c.raw[rng.integers(0, c.N, 600)] + 6.0 * rng.standard_normal((600, c.d))).astype(np.float32)
        args = api.SearchArgs(metric=L2, nprobe=4, exact_ties=1, **WIDE)
        D1, I1 = one.ivfflat_search(q, 10, args)
        # (every distinct row four times: a query is flagged when two of its first 11 distances are equal)
        slice0 = D1[:300]
        assert ((slice0[:, 1:] == slice0[:, :-1]).any(axis=1)).sum() > 256
        check(grp, one, q, 10, args)
        # exact ties off: the merged top-k -- the same distances at every rank
        off = api.SearchArgs(metric=L2, nprobe=4, exact_ties=-1, **WIDE)
        D0, _ = grp.ivfflat_search(q, 10, off)
        assert D0.tobytes() == D1.tobytes()
    finally:
        grp.close()
        one.close()


@pytest.mark.parametrize("placement", ["replicated", "sharded"])
def test_update_across_members_a_vid_named_twice_delete_and_compaction(placement):
    c = LM.Case(144, "float32", L2, seed=91)
    rows = c.raw.copy()
    one = make_one(c, rows)
    grp = make_group(c, 3, placement)
    try:
        fill(grp, placement, rows)
        args = api.SearchArgs(metric=L2, nprobe=4, exact_ties=1, **WIDE)
        check(grp, one, c.q, 10, args)
        # Update: 200 vectors take the rows of others (most change list, many change member); one vid is named twice
        rng = np.random.default_rng(3)
        vids = rng.choice(c.N, 200, replace=False).astype(np.int64)
        vids[-1] = vids[0]
        newv = (rows[rng.integers(0, c.N, 200)] + 0.25 * rng.standard_normal((200, c.d))).astype(np.float32)
        grp.update(vids, newv)
        one.update_batch(vids, newv)
        for j, v in enumerate(vids):      # (the raw rows of the dense stores follow; the sharded rows moved with the update)
            one.raw_write(int(v), newv[j][None])
            if placement != "sharded":
                grp.each(lambda m: m.raw_write(int(v), newv[j][None]))
        q = np.concatenate([c.q, newv[:20] + 0.125])
        check(grp, one, q, 10, args)
        # Delete + compaction
        dead = rng.choice(c.N, c.N // 3, replace=False).astype(np.int64)
        bm = np.zeros((c.N >> 3) + 1, dtype=np.uint8)
        np.bitwise_or.at(bm, dead >> 3, (1 << (dead & 7)).astype(np.uint8))
        grp.delete(dead)
        one.delete(dead)
        grp.each(lambda m: m.bitmap_upload(bm, c.N))
        one.bitmap_upload(bm, c.N)
        check(grp, one, q, 10, args)
        grp.compact_if_need()
        one.compact_if_need()
        check(grp, one, q, 10, args)
    finally:
        grp.close()
        one.close()


def test_a_member_that_answers_an_error_fails_the_call_and_the_next_call_succeeds(plain):
    c, one = plain[L2]
    grp = make_group(c, 3, "replicated", trained=[True, False, True])
    try:
        args = api.SearchArgs(metric=L2, nprobe=4, exact_ties=1, **WIDE)
        with pytest.raises(api.GammaHipError, match="member 1.*not trained"):
            grp.ivfflat_search(c.q, 10, args)
        grp.members[1].ivfflat_set_trained(c.cc)
        fill(grp, "replicated", c.raw)
        check(grp, one, c.q, 10, args)
    finally:
        grp.close()


def test_a_group_set_to_rccl_says_that_ivfflat_calls_use_copies(plain):
    c, one = plain[L2]
    grp = make_group(c, 2, "replicated")
    try:
        fill(grp, "replicated", c.raw)
        grp.set_transport(True)
        args = api.SearchArgs(metric=L2, nprobe=4, exact_ties=1, **WIDE)
        check(grp, one, c.q, 10, args)
        assert "IVFFLAT" in grp.transport()["note"]
    finally:
        grp.close()
