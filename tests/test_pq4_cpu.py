"""CPU: the 4-bit IVFPQ restatement (tests/pq4_ref.py) against the compiled faiss of oracle/_ref -- precomputed table, packed
codes, lists, search_preassigned through the recall heap, training with the 4096-point residual subsample -- every query
bit-identical; and, where oracle/_ref is absent, against the committed goldens (tests/golden/ivfpq4_*.npz), which hold what
the compiled library gave."""
import os

import numpy as np
import pytest

from oracle import binding as B
from tests import gen_golden_pq4 as GG
from tests import pq4_ref as PR

HERE = os.path.dirname(os.path.abspath(__file__))
need_ref = pytest.mark.skipif(not B.have_ref(), reason="oracle/_ref not built (needs the reference tree)")


def _golden(name):
    return dict(np.load(os.path.join(HERE, "golden", "ivfpq4_%s.npz" % name)))


def _check_case(g):
    """the yardstick on a case's trained state and data == what the compiled library produced (dict g)"""
    d, nlist, M, metric = int(g["d"]), int(g["nlist"]), int(g["M"]), int(g["metric"])
    l2 = metric == B.METRIC_L2
    cc, pq, base, q = g["cc"], g["pq"], g["base"], g["q"]
    assert pq.shape == (M, 16, d // M)
    T2 = PR.precompute_table(cc, pq)
    if g["T2"].size:
        assert T2.tobytes() == g["T2"].tobytes(), "precomputed table"
    B.lib().go_set_assign_mode(-1)
    lno, codes = PR.encode(base[:200], cc, pq)
    assert np.array_equal(lno, g["enc_lno"]) and codes.tobytes() == g["enc_codes"].tobytes(), "encode"
    assert codes.shape[1] == PR.code_size(M)
    if M % 2:
        assert (codes[:, -1] >> 4 == 0).all(), "odd M: the last high nibble is 0"
    lno_all, codes_all = PR.encode(base, cc, pq)
    lists = PR.build_lists(lno_all, codes_all, nlist)
    ref_lists = GG.lists_of(g)
    for l in range(nlist):
        assert np.array_equal(lists[l][0], ref_lists[l][0]), "list ids %d" % l
        assert lists[l][1].tobytes() == ref_lists[l][1].tobytes(), "list codes %d" % l
    ix = PR.Index(cc, pq, lists, raw=base)
    R, P = int(g["R"]), int(g["nprobe"])
    cd, ci = PR.coarse(q, cc, P)
    assert cd.tobytes() == g["coarse_dis"].tobytes() and np.array_equal(ci, g["coarse_idx"]), "coarse assignment"
    _, _, st = ix.search(q, R, P, recall_num=R, has_rank=False, l2=l2, min_score=-FLT, max_score=FLT,
                         preassigned=(g["coarse_dis"], g["coarse_idx"]))
    live = g["recall_ids"] != -1
    assert np.array_equal(st["recall_ids"], g["recall_ids"]), "recall-stage labels"
    assert st["recall_dis"][live].tobytes() == g["recall_dis"][live].tobytes(), "recall-stage distances"
    return st


FLT = 3.0e38


def test_pack_layout():
    idx = np.array([[1, 2, 3, 4, 5]], np.uint8)
    assert PR.pack(idx).tolist() == [[0x21, 0x43, 0x05]]
    assert PR.unpack(PR.pack(idx), 5).tolist() == idx.tolist()
    assert PR.code_size(5) == 3 and PR.code_size(32) == 16 and PR.code_size(128) == 64


@pytest.mark.parametrize("name", ["l2_d32", "l2_d64", "ties_d20", "ip_d48"])
def test_yardstick_equals_golden(name):
    st = _check_case(_golden(name))
    if name == "ties_d20":   # the case is there for its ties: at least one query's recall cut goes through equal distances
        g = _golden(name)
        lists = GG.lists_of(g)
        ix = PR.Index(g["cc"], g["pq"], lists)
        cut = 0
        for qi in range(g["q"].shape[0]):
            vals, _ = ix.adc(True, g["q"][qi], g["coarse_idx"][qi], g["coarse_dis"][qi])
            last = st["recall_dis"][qi, -1]
            if st["recall_ids"][qi, -1] != -1 and (vals == last).sum() > (st["recall_dis"][qi] == last).sum():
                cut += 1
        assert cut > 0


@pytest.mark.parametrize("spec", GG.TRAIN_CASES, ids=lambda s: "d%d_l%d_m%d" % s)
def test_training_equals_golden(spec):
    d, nlist, M = spec
    g = np.load(os.path.join(HERE, "golden", "ivfpq4_train.npz"))
    x = PR.clustered(5000, d, 100 + d)
    cc, pq = PR.train(x, nlist, M)
    assert cc.tobytes() == g["cc_%d_%d_%d" % spec].tobytes(), "coarse centroids"
    assert pq.tobytes() == g["pq_%d_%d_%d" % spec].tobytes(), "PQ centroids"


@need_ref
@pytest.mark.parametrize("case", GG.CASES, ids=lambda c: c[0])
def test_yardstick_equals_compiled(case):
    out, _ = GG.ref_case(*case[1:])
    _check_case(out)


@need_ref
@pytest.mark.parametrize("spec", GG.TRAIN_CASES, ids=lambda s: "d%d_l%d_m%d" % s)
def test_training_equals_compiled(spec):
    d, nlist, M = spec
    x = PR.clustered(5000, d, 100 + d)
    r = B.RefIVFPQ(d, nlist, M, 4, B.METRIC_L2)
    r.train(x)
    cc, pq = PR.train(x, nlist, M)
    assert cc.tobytes() == r.coarse_centroids().tobytes(), "coarse centroids"
    assert pq.tobytes() == r.pq_centroids().tobytes(), "PQ centroids"


@need_ref
def test_heap_streams_equal_compiled_on_ties():
    rng = np.random.default_rng(5)
    for trial in range(8):
        n = int(rng.integers(1, 2000))
        vals = rng.integers(0, 5 + 3 * trial, n).astype(np.float32)
        ids = rng.permutation(n).astype(np.int64)
        for l2 in (True, False):
            for k in (1, 7, 64):
                a = PR.heap_stream(vals, ids, k, l2)
                b = PR.heap_stream(vals, ids, k, l2, use_ref=True)
                assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
                a = PR.heap_pop_push_stream(vals, ids, k, l2)
                b = PR.heap_pop_push_stream(vals, ids, k, l2, use_ref=True)
                assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
