"""TEST INFRASTRUCTURE: the yardstick of the OPQ rotation (gamma_hip_opq_*), in the manner of tests/pq4_ref.py.

The rotation's arithmetic is the product's own contract (DESIGN.md "OPQ"), not a restatement of the reference's sgemm_:
every output element is one fp32 accumulator, starting at +0, that takes its d terms in ascending order with one fmaf
each.  apply_chain states that chain on the CPU with an EXACTLY rounded fmaf; everything downstream of the rotated
vectors is the reference's, so the search yardstick is the CPU oracle (oracle/) over the rotated base, with the exact
re-rank done on the raw vectors as GammaIVFPQIndex does it (index/impl/gamma_index_ivfpq.cc:514-566, 646-680)."""
from fractions import Fraction

import numpy as np

from oracle import binding as B

U = 2.0 ** -24   # unit roundoff of fp32


def fma32(a, b, c):
    """round_fp32(a * b + c) for fp32 arrays, rounded ONCE.  The product of two fp32 values is exact in float64; the sum
    is formed in float64 with its rounding error (TwoSum) and, where it is inexact, moved to the neighbour with an odd last
    bit (round to odd), after which the rounding to fp32 is that of the exact value -- a plain float64 product-sum rounds
    twice and is wrong on ties."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)          # s + e == p + c exactly
    fix = (e != 0) & np.isfinite(s) & ((s.view(np.int64) & 1) == 0)
    if fix.any():
        away = (e > 0) == (s > 0)          # the exact value lies further from zero than s
        bits = s.view(np.int64).copy()
        bits[fix] += np.where(away[fix], 1, -1)
        s = bits.view(np.float64)
    return s.astype(np.float32)


def fma32_exact(a, b, c):
    """the same for three Python floats holding fp32 values, through rationals (pins fma32 in tests/test_opq_cpu.py)"""
    v = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if v == 0:
        return np.float32(0.0)
    # round to nearest even at 24 bits (normal range is all the tests use)
    sign = -1 if v < 0 else 1
    m = abs(v)
    ex = 0
    while m >= 2:
        m /= 2
        ex += 1
    while m < 1:
        m *= 2
        ex -= 1
    scaled = m * (1 << 23)
    fl = scaled.numerator // scaled.denominator
    rem = scaled - fl
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and (fl & 1)):
        fl += 1
    return np.float32(sign * float(Fraction(fl, 1 << 23) * (Fraction(2) ** ex)))


def apply_chain(A, x):
    """xt[r, i] = the fmaf chain over j = 0 .. d - 1 of A[i, j] * x[r, j], from +0: the contract of gamma_hip_opq_apply"""
    A = np.ascontiguousarray(A, dtype=np.float32)
    x = np.ascontiguousarray(x, dtype=np.float32)
    d = A.shape[0]
    assert A.shape == (d, d) and x.ndim == 2 and x.shape[1] == d
    acc = np.zeros((x.shape[0], d), dtype=np.float32)
    for j in range(d):
        acc = fma32(np.broadcast_to(A[None, :, j], acc.shape), np.broadcast_to(x[:, j:j + 1], acc.shape), acc)
    return acc


def chain_bound(A, x):
    """|xt_i - exact_i| <= gamma_d * sum_j |A_ij x_j|, gamma_d = d u / (1 - d u): any order of d fp32 fmafs (Higham,
    Accuracy and Stability of Numerical Algorithms, 2nd ed., section 3.1)"""
    d = A.shape[0]
    g = d * U / (1.0 - d * U)
    return g * (np.abs(x.astype(np.float64)) @ np.abs(A.astype(np.float64)).T)


def random_rotation(d, seed):
    """a random orthonormal matrix (numpy QR of a Gaussian matrix), fp32"""
    q, r = np.linalg.qr(np.random.default_rng(seed).standard_normal((d, d)))
    return np.ascontiguousarray(q * np.sign(np.diag(r)), dtype=np.float32)


def mixed_magnitude(d, seed):
    """entries of mixed magnitude and sign, 1e-3 .. 1e3 (not a rotation: the rotation kernel does not care)"""
    rng = np.random.default_rng(seed)
    return (rng.choice([-1.0, 1.0], (d, d)) * 10.0 ** rng.uniform(-3, 3, (d, d))).astype(np.float32)


def signed_permutation(d, seed):
    rng = np.random.default_rng(seed)
    A = np.zeros((d, d), dtype=np.float32)
    A[np.arange(d), rng.permutation(d)] = rng.choice([-1.0, 1.0], d)
    return A


def clustered(n, d, seed, k=24):
    """Gaussian clusters (real-valued: exact distance ties do not occur, which search_ref checks)"""
    rng = np.random.default_rng(seed)
    cen = 3.0 * np.random.default_rng(777 + d).standard_normal((k, d))
    return (cen[rng.integers(0, k, n)] + rng.standard_normal((n, d))).astype(np.float32)


def build_oracle(base_rot, nlist, M, metric, ntrain=3000, raw=None):
    """trained state from the rotated set (gamma_index_ivfpq.cc:336-346 trains on the rotated vectors) and an oracle index
    over the rotated base; raw: what its re-rank reads (None: nothing -- search_ref re-ranks on the raw base itself)"""
    d = base_rot.shape[1]
    cc, pq = B.ivfpq_train(base_rot[:min(len(base_rot), ntrain)], nlist, M)
    o = B.OracleIVFPQ(d, nlist, M, 8, metric)
    o.set_trained(cc, pq, None)
    B.lib().go_set_assign_mode(-1)
    assert o.add(base_rot)
    if raw is not None:
        o.set_raw(raw)
    return o, cc, pq


def search_ref(o, base_raw, q_raw, q_rot, k, nprobe, recall_num, has_rank, metric, min_score=None, max_score=None,
               docids_bitmap=None, range_filters=None, coarse_mode=-1):
    """(D, I, stages) of a search with a rotation: coarse and recall stage from the oracle over the ROTATED queries
    (has_rank off); with has_rank the final table is compute_dis on the RAW query and the raw rows of the recall stage's
    candidates (B.flat_search over base[cand]: the oracle's own exact distances and k-heap), the score window on the exact
    distance.  The oracle's recall stage comes back sorted, compute_dis feeds the k-heap in the recall heap's array order:
    the two agree when a query's candidates have pairwise distinct exact distances, which is asserted."""
    mk = lambda: B.make_ctx(docids_bitmap=docids_bitmap, range_filters=range_filters, min_score=min_score, max_score=max_score)
    D, I, st = o.search(q_rot, k, nprobe, recall_num=recall_num, has_rank=False, metric=metric, ctx=mk(),
                        coarse_mode=coarse_mode, want_stages=True)
    if not has_rank:
        return D, I, st
    l2 = metric == B.METRIC_L2
    D = np.full((len(q_raw), k), np.finfo(np.float32).max if l2 else -np.finfo(np.float32).max, dtype=np.float32)
    I = np.full((len(q_raw), k), -1, dtype=np.int64)
    window = B.make_ctx(min_score=min_score, max_score=max_score)
    wide = B.make_ctx(min_score=-3e38, max_score=3e38)
    for qi in range(len(q_raw)):
        cand = st["recall_ids"][qi]
        cand = cand[cand >= 0]
        if not len(cand):
            continue
        rows = base_raw[cand]
        De, _ = B.flat_search(rows, q_raw[qi:qi + 1], len(cand), metric, wide)
        assert len(np.unique(De[0].view(np.uint32))) == len(cand), "equal exact distances among the candidates of query %d" % qi
        kk = min(k, len(cand))
        Dk, Ik = B.flat_search(rows, q_raw[qi:qi + 1], kk, metric, window)
        ok = Ik[0] >= 0
        D[qi, :ok.sum()] = Dk[0][ok]
        I[qi, :ok.sum()] = cand[Ik[0][ok]]
    return D, I, st


def pick_queries(o, base_raw, A, stream, nq, k, nprobe, recall_num, metric, docids_bitmap=None, range_filters=None):
    """the first nq vectors of `stream` that meet search_ref's condition on the inputs -- the recall stage's candidates have
    pairwise distinct exact distances to the raw query -- decided on the CPU alone (rotation by apply_chain, candidates from
    the oracle).  Two of a few dozen fp32 distances coincide for about one real-valued query in a thousand; such a query's
    order inside the tie is the reference heap's, which the sorted recall stage of the oracle cannot tell."""
    stream = np.ascontiguousarray(stream, dtype=np.float32)
    ctx = B.make_ctx(docids_bitmap=docids_bitmap, range_filters=range_filters, min_score=-3e38, max_score=3e38)
    _, _, st = o.search(apply_chain(A, stream), k, nprobe, recall_num=recall_num, has_rank=False, metric=metric, ctx=ctx,
                        want_stages=True)
    wide = B.make_ctx(min_score=-3e38, max_score=3e38)
    good = []
    for qi in range(len(stream)):
        cand = st["recall_ids"][qi]
        cand = cand[cand >= 0]
        if len(cand):
            De, _ = B.flat_search(base_raw[cand], stream[qi:qi + 1], len(cand), metric, wide)
            if len(np.unique(De[0].view(np.uint32))) != len(cand):
                continue
        good.append(qi)
        if len(good) == nq:
            return stream[good]
    raise AssertionError("the stream holds fewer than %d queries with distinct candidate distances" % nq)


def anisotropic(n, d, seed, decay):
    """the training sets of tests/golden/opq_train.npz: Gaussian with geometrically decaying standard deviations
    (decay ** j), then a fixed random rotation -- correlated dimensions of very unequal variance, what OPQ is for"""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((n, d)) * (decay ** np.arange(d))[None, :]
    return np.ascontiguousarray(z @ random_rotation(d, seed + 1).astype(np.float64).T, dtype=np.float32)


def rotate64(A, x):
    """x A^T in float64, summed term by term in ascending order (no BLAS: the same bits on every machine)"""
    A = np.asarray(A, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    acc = np.zeros((x.shape[0], A.shape[0]))
    for j in range(A.shape[1]):
        acc += x[:, j:j + 1] * A[None, :, j]
    return acc


def pq_error(A, x, M, niter=25):
    """the fixed CPU evaluation of a rotation's quality: the centred set rotated in float64, one B.kmeans (256 centroids,
    niter iterations) per sub-space, the mean squared reconstruction error"""
    x = np.asarray(x, dtype=np.float64)
    xr = rotate64(A, x - x.mean(axis=0, keepdims=True)).astype(np.float32)
    d = xr.shape[1]
    ds = d // M
    err = 0.0
    for m in range(M):
        sub = np.ascontiguousarray(xr[:, m * ds:(m + 1) * ds])
        cen, _ = B.kmeans(sub, 256, niter)
        s64, c64 = sub.astype(np.float64), cen.astype(np.float64)
        best = np.full(len(sub), np.inf)
        for c0 in range(0, 256, 32):                   # exact squared distances, 32 centroids at a time
            dd = ((s64[:, None, :] - c64[None, c0:c0 + 32, :]) ** 2).sum(axis=2)
            best = np.minimum(best, dd.min(axis=1))
        err += float(best.sum())
    return err / len(x)


def orthonormality_defect(A):
    A = np.asarray(A, dtype=np.float64)
    return float(np.abs(A @ A.T - np.eye(A.shape[0])).max())


OPQ_TRAIN_CASES = [dict(name="d32", d=32, M=4, n=10000, seed=41, decay=0.8),
                   dict(name="d64", d=64, M=8, n=10000, seed=43, decay=0.9)]
