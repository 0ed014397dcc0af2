"""CPU: the binary IVF restatement (tests/binivf_ref.py) on the oracle's heap streams and k-means against the compiled faiss
of oracle/_ref, on tie-heavy input (Hamming distances are small integers: nearly every heap sees exact ties; +-1 training
data gives exact ties in the k = 1 assignment), and against the committed golden (tests/golden/binivf_train.npz)."""
import os

import numpy as np
import pytest

from oracle import binding as B
from tests import binivf_ref as BR

HERE = os.path.dirname(os.path.abspath(__file__))
need_ref = pytest.mark.skipif(not B.have_ref(), reason="oracle/_ref not built (needs the reference tree)")


def _lists(n, nbits, nlist, seed):
    rng = np.random.default_rng(seed)
    codes = BR.clustered_codes(n, nbits, 8, flip=0.05, seed=seed, dup_frac=0.2)
    cc = codes[rng.choice(n, nlist, replace=False)]
    return codes, cc, BR.assign_lists(codes, cc)


def test_hamming_and_bit_order():
    a = np.array([[0b00000001, 0xff]], np.uint8)
    assert BR.hamming(a[0], np.array([[0, 0], [1, 0xff], [0xff, 0xff]], np.uint8)).tolist() == [9, 0, 7]
    x = BR.binary_to_real(np.array([[0b00000101]], np.uint8))
    assert x.tolist() == [[1, -1, 1, -1, -1, -1, -1, -1]]
    # real_to_binary: only > 0 sets a bit; an exact 0.0 (as many +1 as -1 averaged) gives 0
    assert BR.real_to_binary(np.array([[0.5, 0.0, -0.0, -1, 1e-30, 0, 0, 2]], np.float32)).tolist() == [[0b10010001]]


def test_score_window_default_excludes_distance_zero():
    codes, cc, lists = _lists(300, 64, 4, 3)
    x = codes[:5]
    D, I = BR.search(lists, cc, x, 10, 4)
    assert (D > 0).all()
    D2, I2 = BR.search(lists, cc, x, 10, 4, min_score=0, max_score=1e4)
    assert (D2[:, 0] == 0).all()


def test_nprobe_rule():
    assert BR.resolve_nprobe(5, 16) == 5
    assert BR.resolve_nprobe(16, 16) == 16
    assert BR.resolve_nprobe(17, 16) == 20
    assert BR.resolve_nprobe(0, 16) == 20
    assert BR.resolve_nprobe(-3, 100) == 20


@need_ref
@pytest.mark.parametrize("k", [1, 3, 10, 64, 300])
def test_heap_streams_restated_equal_compiled_on_ties(k):
    rng = np.random.default_rng(k)
    for trial in range(6):
        n = int(rng.integers(1, 3000))
        vals = rng.integers(0, 6 + trial * 4, n).astype(np.float32)   # few distinct values: ties everywhere
        ids = rng.permutation(n).astype(np.int64)
        for fn in (BR.heap_replace_top_stream, BR.heap_pop_push_stream):
            gv, gi = fn(vals, ids, k)
            rv, ri = fn(vals, ids, k, use_ref=True)
            assert gv.tobytes() == rv.tobytes() and np.array_equal(gi, ri), (fn.__name__, k, n)


@need_ref
@pytest.mark.parametrize("nbits,nlist,nprobe", [(64, 16, 4), (256, 64, 20), (32, 8, 20)])
def test_coarse_and_scan_restated_equal_compiled(nbits, nlist, nprobe):
    codes, cc, lists = _lists(3000, nbits, nlist, nbits + nlist)
    x = np.concatenate([codes[:20], BR.clustered_codes(20, nbits, 8, seed=99)])
    P = BR.resolve_nprobe(nprobe, nlist)
    gd, gi = BR.coarse(x, cc, P)
    rd, ri = BR.coarse(x, cc, P, use_ref=True)
    assert np.array_equal(gd, rd) and np.array_equal(gi, ri)
    if P > nlist:
        assert (gi[:, nlist:] == -1).all() and (gd[:, nlist:] == BR.INT32_MAX).all()
    f = BR.Filter(deleted=range(0, 3000, 7), ranges=[(range(100, 2500), True)])
    for k in (1, 10, 100):
        for lo, hi in ((None, None), (0, 1e4), (3, 9)):
            a = BR.search(lists, cc, x, k, nprobe, lo, hi, filt=f)
            b = BR.search(lists, cc, x, k, nprobe, lo, hi, filt=f, use_ref=True)
            assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])


@need_ref
@pytest.mark.parametrize("nbits,nlist", [(64, 16), (256, 16), (512, 16), (64, 256), (256, 256)])
def test_training_restated_equals_compiled(nbits, nlist):
    n = nlist * (60 if nlist <= 16 else 40)
    codes = BR.clustered_codes(n, nbits, max(2, nlist // 2), flip=0.03, seed=nbits + nlist, dup_frac=0.2)
    assert np.array_equal(BR.train(codes, nlist), BR.train(codes, nlist, use_ref=True))


@need_ref
def test_training_nx_equals_nlist_restated_equals_compiled():
    codes = BR.clustered_codes(32, 128, 4, seed=5, dup_frac=0.3)
    a, b = BR.train(codes, 32), BR.train(codes, 32, use_ref=True)
    assert np.array_equal(a, b) and np.array_equal(a, codes)


def test_training_restatement_matches_golden():
    g = np.load(os.path.join(HERE, "golden", "binivf_train.npz"))
    names = sorted({k[:-6] for k in g.files if k.endswith("_codes")})
    assert len(names) >= 4
    for name in names:
        nlist = int(g[name + "_nlist"])
        assert np.array_equal(BR.train(g[name + "_codes"], nlist), g[name + "_cc"]), name
