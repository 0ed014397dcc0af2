"""CPU: the yardstick of the OPQ rotation (tests/opq_ref.py) is pinned -- its fmaf is rounded once, its chain stays
within the derived bound and is exact where the data makes every order exact."""
import os
import struct

import numpy as np

from tests import opq_ref as OR


def test_fma32_rounds_once():
    # a * b = 2^-24 - 2^-70, c = 1 + 2^-23: the exact sum lies just BELOW the midpoint of 1 + 2^-23 and 1 + 2^-22.  float64
    # rounds it onto the midpoint, and rounding that to fp32 (ties to even) gives 1 + 2^-22 -- the double rounding
    a = np.array([2.0 ** -12 * (1 + 2.0 ** -23)], np.float32)
    b = np.array([2.0 ** -12 * (1 - 2.0 ** -23)], np.float32)
    c = np.array([1 + 2.0 ** -23], np.float32)
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    assert naive[0] == np.float32(1 + 2.0 ** -22)
    assert OR.fma32(a, b, c)[0] == np.float32(1 + 2.0 ** -23)
    assert OR.fma32_exact(a[0], b[0], c[0]) == np.float32(1 + 2.0 ** -23)
    # the mirror image: just above the midpoint below an even neighbour
    assert OR.fma32(a, -b, -c)[0] == np.float32(-(1 + 2.0 ** -23))
    # random operands of mixed magnitude against rationals
    rng = np.random.default_rng(0)
    n = 1500
    a = rng.standard_normal(n).astype(np.float32)
    b = rng.standard_normal(n).astype(np.float32)
    c = (rng.standard_normal(n) * 10.0 ** rng.uniform(-8, 8, n)).astype(np.float32)
    r = OR.fma32(a, b, c)
    for i in range(n):
        assert OR.fma32_exact(a[i], b[i], c[i]).tobytes() == r[i].tobytes(), i


def test_chain_is_the_chain_and_within_the_bound():
    for d, n in ((15, 33), (20, 65), (32, 1), (160, 40)):
        for A in (OR.random_rotation(d, d), OR.mixed_magnitude(d, d + 1)):
            x = OR.clustered(n, d, d + 2)
            xt = OR.apply_chain(A, x)
            # element (0, d - 1) spelled out with the rational fmaf
            acc = np.float32(0.0)
            for j in range(d):
                acc = OR.fma32_exact(A[d - 1, j], x[0, j], acc)
            assert acc.tobytes() == xt[0, d - 1].tobytes()
            exact = x.astype(np.float64) @ A.astype(np.float64).T
            assert (np.abs(xt.astype(np.float64) - exact) <= OR.chain_bound(A, x)).all()


def test_chain_is_exact_on_integers_under_a_signed_permutation():
    rng = np.random.default_rng(3)
    A = OR.signed_permutation(32, 5)
    assert np.array_equal(A @ A.T, np.eye(32, dtype=np.float32))
    x = rng.integers(-8, 9, (50, 32)).astype(np.float32)
    assert np.array_equal(OR.apply_chain(A, x), x @ A.T)


def test_golden_errors_reproduce_with_the_evaluation():
    """pins opq_ref.pq_error: the golden's recorded figures (tests/gen_golden_opq.py) come out of it again"""
    G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "opq_train.npz"))
    c = OR.OPQ_TRAIN_CASES[0]
    x = OR.anisotropic(c["n"], c["d"], c["seed"], c["decay"])
    assert np.isclose(OR.pq_error(np.eye(c["d"], dtype=np.float32), x, c["M"]), float(G[c["name"] + "_err_identity"]), rtol=1e-6, atol=0)
    assert np.isclose(OR.pq_error(G[c["name"] + "_A"][0], x, c["M"]), G[c["name"] + "_err"][0], rtol=1e-6, atol=0)
    assert np.isclose(OR.orthonormality_defect(G[c["name"] + "_A"][0]), G[c["name"] + "_defect"][0], rtol=1e-6, atol=0)
    for cc in OR.OPQ_TRAIN_CASES:                      # the condition that makes the GPU test mean something
        assert G[cc["name"] + "_err"].max() <= 0.8 * float(G[cc["name"] + "_err_identity"])


# ---- the "LTra" record of ivfpq.index (index/gamma_index_io.cc:225-260) through host/iwpq_io.cc --------------------------------
def _base_file(tmp_path, d=8, nlist=2, M=2):
    from gamma_amd import plugin
    rng = np.random.default_rng(1)
    cc = rng.standard_normal((nlist, d)).astype(np.float32)
    pq = rng.standard_normal((M, 256, d // M)).astype(np.float32)
    codes = rng.integers(0, 256, (3, M)).astype(np.uint8)   # list 0 holds three entries, list 1 none
    ids = np.arange(3, dtype=np.int64)
    path = str(tmp_path / "plain.index")
    assert plugin.iwpq_write(path, d, 0, 1, 1, cc, pq, [3, 0], codes, ids) == 0
    return path, open(path, "rb").read()


def _record(A, d_in, d_out):
    return (b"LTra" + b"\x00" + struct.pack("<Q", A.size) + A.tobytes() + struct.pack("<Q", 0) + struct.pack("<ii", d_in, d_out)
            + b"\x01")


def test_ltra_record_round_trips_and_mismatches_are_rejected(tmp_path):
    from gamma_amd import plugin
    d = 8
    path, plain = _base_file(tmp_path, d)
    at = plain.index(b"ilar")
    assert plain.count(b"ilar") == 1
    assert plugin.iwpq_read_opq(path, d) == (0, None)
    A = OR.random_rotation(d, 2)
    with_rec = str(tmp_path / "opq.index")
    assert plugin.iwpq_rewrite_opq(path, with_rec, A) == 0
    assert open(with_rec, "rb").read() == plain[:at] + _record(A, d, d) + plain[at:]
    rc, back = plugin.iwpq_read_opq(with_rec, d)
    assert rc == 0 and back.tobytes() == A.tobytes()
    again = str(tmp_path / "again.index")
    assert plugin.iwpq_rewrite_opq(with_rec, again, None) == 0          # and without it: the plain file again
    assert open(again, "rb").read() == plain
    # a record whose d_in / d_out disagree with d, or whose matrix is not d x d, is a bad file
    bad = str(tmp_path / "bad.index")
    for rec in (_record(A, d + 1, d), _record(A, d, d - 1), _record(A[:4], d, d)):
        open(bad, "wb").write(plain[:at] + rec + plain[at:])
        assert plugin.iwpq_read_opq(bad, d)[0] < 0
    assert plugin.iwpq_rewrite_opq(path, bad, A[:4]) < 0               # the writer refuses a matrix that is not d x d
