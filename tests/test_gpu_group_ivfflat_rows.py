"""GPU: the IVFFLAT search of the in-process group over members with float16 / uint8 / int8 stores (gamma_hip_group_ivfflat_search
after gamma_hip_set_ivfflat_narrow_rows on every member, and gamma_hip_set_sparse_narrow_rows where the rows are sharded with
their lists).  Every member lives on device 0.  The group keeps taking fp32 vectors, the members convert.  The
yardstick is ONE handle with a dense store of the type, fed the same calls and compared strictly (compare_exact: labels and
distance bits at every rank), and for two members the CPU oracle over the widened rows and the handle's own lists."""
import numpy as np
import pytest

from gamma_amd import api
from oracle import binding as B
from tests import ivfflat_lm_data as LM
from tests import ivfflat_rows_data as R
from tests import ivfflat_shard_ref as SR
from tests import ivfflat_shard_rows_data as RD
from tests.parity import compare_exact

pytestmark = pytest.mark.gpu

L2, IP = B.METRIC_L2, B.METRIC_IP
WIDE = SR.WIDE
PLACEMENTS = ["replicated", "sharded", "replicate"]      # raw rows replicated | raw rows sharded | lists replicated
DTYPE = pytest.mark.parametrize("dtype", RD.DTYPES)
UNSTORABLE = {"float16": (1e6, "binary16"), "uint8": (0.5, "not exactly storable"), "int8": (200.0, "not exactly storable")}


def _init(m, c, dtype, sharded):
    m.ivfflat_init(c.d, c.nlist, c.metric)
    m.ivfflat_set_trained(c.cc)
    m.raw_init(c.d, dtype)
    if dtype != "float32":
        m.set_ivfflat_narrow_rows(True)
        if sharded:
            m.set_sparse_narrow_rows(True)


def make_group(c, W, placement, dtype, dtypes=None):
    grp = api.GammaHipGroup([0] * W)
    for i, m in enumerate(grp.members):
        _init(m, c, dtypes[i] if dtypes else dtype, placement == "sharded")
    if placement == "replicate":
        grp.set_placement(True)
    if placement == "sharded":
        grp.set_raw_placement(True)
    grp.set_owners(None)
    return grp


def fill(grp, placement, rows):
    for i0 in range(0, len(rows), 1000):
        grp.add(rows[i0:i0 + 1000], i0)
        if placement != "sharded":
            grp.each(lambda m: m.raw_append(rows[i0:i0 + 1000]))


def make_one(c, dtype, rows):
    g = api.GammaHip(0)
    _init(g, c, dtype, False)
    for i0 in range(0, len(rows), 1000):
        g.add(rows[i0:i0 + 1000], i0)
        g.raw_append(rows[i0:i0 + 1000])
    return g


def check(grp, one, q, k, args):
    D1, I1 = one.ivfflat_search(q, k, args)
    D, I = grp.ivfflat_search(q, k, args)
    compare_exact(D1, I1, D, I)
    return D, I


def oracle_of(c, one, held):
    """the CPU oracle over the lists as the one handle holds them (its own coarse assignment) and the rows `held`"""
    o = B.OracleIVFPQ(c.d, c.nlist, 1, 8, c.metric)
    o.set_trained(c.cc, np.zeros((256, c.d), np.float32), None)
    for l in range(c.nlist):
        ids, _ = one.get_list(l)
        if len(ids):
            assert o.add_keys(l, ids, np.zeros((len(ids), 1), np.uint8))
    o.set_raw(held)
    return o


@pytest.mark.parametrize("placement", PLACEMENTS)
@DTYPE
@pytest.mark.parametrize("W,metric", [(2, L2), (3, IP)])
def test_group_equals_one_handle_of_the_type(W, metric, dtype, placement):
    c = RD.case(128, dtype, metric)
    one = make_one(c, dtype, c.base)
    grp = make_group(c, W, placement, dtype)
    try:
        fill(grp, placement, c.base)
        assert all(m.raw_elem_bytes() == R.ESZ[dtype] for m in grp.members)
        args = api.SearchArgs(metric=metric, nprobe=4, exact_ties=1, **WIDE)
        rng = np.random.default_rng(W)
        big = (c.W[rng.integers(0, c.N, 300)] + 0.5 * rng.standard_normal((300, c.d))).astype(np.float32)
        for nq in (1, 7, 64, 300):      # nq 1 leaves empty slices
            D, I = check(grp, one, big[:nq], 10, args)
        if placement == "sharded":
            st = [m.raw_sparse_stats()["live"] for m in grp.members]
            assert sum(st) == c.N and all(s < c.N for s in st)      # every row once, at the owner of its list
        if W == 2:
            held = c.W.copy()
            o = oracle_of(c, one, held)
            D0, I0 = B.ivfflat_search(o, big, 10, 4, metric, B.make_ctx(**WIDE))
            compare_exact(D0, I0, D, I)
    finally:
        grp.close()
        one.close()


@pytest.mark.parametrize("placement", ["replicated", "sharded"])
@DTYPE
def test_the_tie_phase_runs(dtype, placement):
    """integer-valued rows, every distinct row four times: most queries go through the flag rule and the replay"""
    c = RD.tie_case(dtype, L2)
    one = make_one(c, dtype, c.base)
    grp = make_group(c, 2, placement, dtype)
    try:
        fill(grp, placement, c.base)
        args = api.SearchArgs(metric=L2, nprobe=4, exact_ties=1, **WIDE)
        for m in grp.members:
            m.tie_stats(reset=True)
        D, I = check(grp, one, c.q, 10, args)
        assert ((D[:, 1:] == D[:, :-1]).any(axis=1)).sum() > 0      # equal distances inside the results: flagged queries
        st = [m.tie_stats() for m in grp.members]
        assert sum(s["cut_ties"] + s["replayed"] for s in st) > 0, st
        o = oracle_of(c, one, c.W.copy())
        D0, I0 = B.ivfflat_search(o, c.q, 10, 4, L2, B.make_ctx(**WIDE))
        compare_exact(D0, I0, D, I)
        # exact ties off: the merged top-k -- the same distances at every rank
        off = api.SearchArgs(metric=L2, nprobe=4, exact_ties=-1, **WIDE)
        D1, _ = one.ivfflat_search(c.q, 10, args)
        Doff, _ = grp.ivfflat_search(c.q, 10, off)
        assert Doff.tobytes() == D1.tobytes()
    finally:
        grp.close()
        one.close()


@pytest.mark.parametrize("placement", ["replicated", "sharded"])
@DTYPE
def test_update_across_members_a_vid_named_twice_delete_and_compaction(dtype, placement):
    c = LM.Case(144, dtype, L2, seed=91)
    rows = c.base.copy()
    one = make_one(c, dtype, rows)
    grp = make_group(c, 3, placement, dtype)
    try:
        fill(grp, placement, rows)
        args = api.SearchArgs(metric=L2, nprobe=4, exact_ties=1, **WIDE)
        check(grp, one, c.q, 10, args)
        # Update: 200 vectors take the rows of others (most change list, many change member); one vid is named twice
        rng = np.random.default_rng(3)
        vids = rng.choice(c.N, 200, replace=False).astype(np.int64)
        vids[-1] = vids[0]
        newv = rows[rng.integers(0, c.N, 200)].copy()
        if dtype == "float16":
            newv += (0.25 * rng.standard_normal((200, c.d))).astype(np.float32)
        grp.update(vids, newv)
        one.update_batch(vids, newv)
        for j, v in enumerate(vids):      # (the raw rows of the dense stores follow; the sharded rows moved with the update)
            one.raw_write(int(v), newv[j][None])
            if placement != "sharded":
                grp.each(lambda m: m.raw_write(int(v), newv[j][None]))
        q = np.concatenate([c.q, R.widened(newv[:20], dtype) + 0.125])
        check(grp, one, q, 10, args)
        if placement == "sharded":
            assert sum(m.raw_sparse_stats()["live"] for m in grp.members) == c.N
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


def test_mixed_element_types_are_refused_by_set_raw_placement():
    c = RD.case(24, "uint8", IP)
    for dtypes in (["uint8", "int8"], ["float16", "float32"], ["uint8", "uint8", "float16"]):
        grp = api.GammaHipGroup([0] * len(dtypes))
        try:
            for m, dt in zip(grp.members, dtypes):
                _init(m, c, dt, True)
            with pytest.raises(api.GammaHipError, match="raw stores differ"):
                grp.set_raw_placement(True)
            assert not grp.raw_placement()
        finally:
            grp.close()


@DTYPE
def test_a_row_a_store_cannot_hold_fails_the_call_with_no_member_touched(dtype):
    c = RD.case(24, dtype, IP)
    one = make_one(c, dtype, c.base[:2000])
    grp = make_group(c, 3, "sharded", dtype)
    try:
        fill(grp, "sharded", c.base[:2000])
        args = api.SearchArgs(metric=IP, nprobe=4, exact_ties=1, **WIDE)
        D, I = check(grp, one, c.q, 10, args)
        value, msg = UNSTORABLE[dtype]
        bad = c.base[2000:2100].copy()
        bad[70, 7] = value
        live = [m.raw_sparse_stats()["live"] for m in grp.members]
        sizes = [grp.list_size(l) for l in range(c.nlist)]
        for call in (lambda: grp.add(bad, 2000), lambda: grp.update(np.arange(100, dtype=np.int64), bad),
                     lambda: grp.raw_put(np.arange(100, dtype=np.int64), bad)):
            with pytest.raises(api.GammaHipError, match=msg):
                call()
            assert [m.raw_sparse_stats()["live"] for m in grp.members] == live
            assert [grp.list_size(l) for l in range(c.nlist)] == sizes
            D2, I2 = grp.ivfflat_search(c.q, 10, args)
            assert D2.tobytes() == D.tobytes() and I2.tobytes() == I.tobytes()
        # the same rows without the bad value are taken
        grp.add(c.base[2000:2100], 2000)
        one.add(c.base[2000:2100], 2000)
        one.raw_append(c.base[2000:2100])
        check(grp, one, c.q, 10, args)
    finally:
        grp.close()
        one.close()
