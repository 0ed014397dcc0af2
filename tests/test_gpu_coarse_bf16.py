"""GPU: the coarse quantizer's filter on the bf16 matrix pipe (csrc/coarse.hip, "bf16 filter").  set_coarse_fused(1)
-- the default -- must give the bytes of set_coarse_fused(2) (fp32 filter) and set_coarse_fused(0) (distance matrix),
with exact ties on and off, on plain data, on data whose exact keys crowd the margin band, on data whose band swallows
the survivor lists (the handle then switches itself to the fp32 filter), and outside the filter's magnitude domain."""
import numpy as np
import pytest

from gamma_amd import api, synth
from oracle import binding as B
from tests import fixtures

pytestmark = pytest.mark.gpu

WIDE = dict(min_score=-3e38, max_score=3e38)


def _handle(cc):
    nlist, d = cc.shape
    M = d // 8
    pq = np.random.default_rng(1).standard_normal((M, 256, d // M)).astype(np.float32)
    g = api.GammaHip(0)
    g.ivfpq_init(d, nlist, M, 8, api.METRIC_L2, 100)
    g.ivfpq_set_trained(cc, pq, None)
    return g


def _runner(g, x, P):
    import torch
    dev = torch.device("cuda", 0)
    nq = x.shape[0]
    dx = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)

    def run(mode, ties, cap=128):
        g.set_coarse_fused(mode, cap)
        args = api.SearchArgs(metric=api.METRIC_L2, nprobe=P, coarse_mode=1, exact_ties=1 if ties else -1, **WIDE)
        cd = torch.empty((nq, P), dtype=torch.float32, device=dev)
        ci = torch.empty((nq, P), dtype=torch.int32, device=dev)
        g.ivfpq_coarse_device(dx.data_ptr(), nq, args, cd.data_ptr(), ci.data_ptr())
        g.synchronize()
        return cd.cpu().numpy(), ci.cpu().numpy()

    return run


def _same_in_all_modes(run, tag):
    out = {}
    for ties in (True, False):
        D0, I0 = run(0, ties)
        for mode in (2, 1):
            D, I = run(mode, ties)
            assert D0.tobytes() == D.tobytes(), (tag, mode, ties)
            assert np.array_equal(I0, I), (tag, mode, ties)
        out[ties] = (D0, I0)
    return out


def _plain_data(d, nlist, P, nq):
    rng = np.random.default_rng(d + nlist + P)
    cc = (rng.standard_normal((nlist, d)) * 20).astype(np.float32)
    cc[5] = cc[600]                                   # duplicate centroids
    cc[nlist - 1] = cc[700]
    cc[9] = 0                                         # an all-zero centroid
    x = cc[rng.integers(0, nlist, nq)] + (rng.standard_normal((nq, d)) * 12).astype(np.float32)
    x[3] = cc[5]                                      # a query equal to a centroid (twice)
    x[4] = 0                                          # an all-zero query
    return cc, x


@pytest.mark.parametrize("d,nlist,P,nq", [(128, 2048, 32, 4100), (32, 2100, 8, 4100), (64, 4100, 64, 4200),
                                          (96, 2304, 20, 4100)])
def test_bf16_filter_matches_fp32_and_matrix_paths(d, nlist, P, nq):
    cc, x = _plain_data(d, nlist, P, nq)
    g = _handle(cc)
    try:
        run = _runner(g, x, P)
        _same_in_all_modes(run, "plain")
        st = g.coarse_filter_stats()
        assert st["queries"] >= 2 * nq and st["backoffs"] == 0, st   # the bf16 chain ran, and stayed on
        D2, I2 = run(2, True)
        for cap in (40, 1):                                          # survivor lists overflow: repair kernels
            D1, I1 = run(1, True, cap)
            assert D2.tobytes() == D1.tobytes() and np.array_equal(I2, I1), cap
    finally:
        g.close()


def test_bf16_filter_integer_valued_data():
    """sift-like integers: the three bf16 products are exact, exact ties are frequent -- the rows handed to the heap
    replay and the final assignment are those of the fp32 filter."""
    d, nlist, P, nq = 128, 2048, 32, 4100
    base = synth.sift_like(20000, d=d, seed=21)
    cc = base[np.random.default_rng(3).choice(len(base), nlist, replace=False)].copy()
    x = synth.sift_like(nq, d=d, seed=22)
    g = _handle(cc)
    try:
        run = _runner(g, x, P)
        rows = {}
        outs = {}
        for mode in (2, 1):
            g.tie_stats(reset=True)
            outs[mode] = run(mode, True)
            rows[mode] = g.tie_stats()["coarse_rows"]
        assert outs[1][0].tobytes() == outs[2][0].tobytes() and np.array_equal(outs[1][1], outs[2][1])
        assert rows[1] == rows[2], rows
        D0, I0 = run(0, True)
        assert D0.tobytes() == outs[1][0].tobytes() and np.array_equal(I0, outs[1][1])
    finally:
        g.close()


def _band_data(shift):
    """centroids in clusters of 3 P near-copies, each 1, 2 or 4 ulps off in one component: many exact keys sit within
    the margin band around the P-th"""
    d, nlist, P, nq = 128, 2048, 32, 4100
    rng = np.random.default_rng(77)
    ncl = (nlist + 3 * P - 1) // (3 * P)
    centres = (rng.standard_normal((ncl, d)) * 4).astype(np.float32) + np.float32(shift)
    cc = np.repeat(centres, 3 * P, axis=0)[:nlist].copy()
    comp = rng.integers(0, d, nlist)
    ulps = rng.choice([1, 2, 4], nlist)
    v = cc[np.arange(nlist), comp]
    for _ in range(4):
        step = ulps > 0
        v = np.where(step, np.nextafter(v, np.float32(np.inf)), v)
        ulps = ulps - 1
    cc[np.arange(nlist), comp] = v
    x = centres[rng.integers(0, ncl, nq)] + (rng.standard_normal((nq, d)) * 2).astype(np.float32)
    return cc, x.astype(np.float32), P


def test_bf16_filter_margin_band_of_near_copies():
    cc, x, P = _band_data(0.0)
    g = _handle(cc)
    try:
        _same_in_all_modes(_runner(g, x, P), "band")
    finally:
        g.close()


def test_bf16_filter_backs_off_when_the_band_swallows_the_lists():
    """norms >> distances (every component + 1000): the margin keeps most of a strip, every list overflows.  Results
    stay those of the other modes, and the handle switches itself to the fp32 filter (coarse_filter_stats)."""
    cc, x, P = _band_data(1000.0)
    g = _handle(cc)
    try:
        run = _runner(g, x, P)
        D0, I0 = run(0, True)
        D2, I2 = run(2, True)
        assert D0.tobytes() == D2.tobytes() and np.array_equal(I0, I2)
        st0 = g.coarse_filter_stats()
        assert st0["backoffs"] == 0
        for call in range(4):
            D1, I1 = run(1, True)
            assert D0.tobytes() == D1.tobytes() and np.array_equal(I0, I1), call
        st = g.coarse_filter_stats()
        assert st["backoffs"] >= 1 and st["fp32_calls_left"] > 0, st
        assert st["given_up"] > st["queries"] // 8, st
        assert st["queries"] < 4 * x.shape[0], st          # the later calls did not run the bf16 chain
    finally:
        g.close()


@pytest.mark.parametrize("scale", [1e-18, 1e15])
def test_bf16_filter_magnitudes(scale):
    cc, x = _plain_data(128, 2048, 32, 4100)
    cc = (cc * np.float32(scale)).astype(np.float32)
    x = (x * np.float32(scale)).astype(np.float32)
    assert np.isfinite(cc).all() and np.isfinite(x).all()
    g = _handle(cc)
    try:
        _same_in_all_modes(_runner(g, x, 32), scale)
    finally:
        g.close()


def test_whole_search_bf16_coarse_equals_matrix_path():
    d, nlist, M, N, nq = 32, 2048, 8, 40000, 4200
    rng = np.random.default_rng(7)
    base = synth.sift_like(N, d=d, seed=11)
    q = synth.sift_like(nq, d=d, seed=12)
    cc = base[rng.choice(N, nlist, replace=False)].copy()
    pq = (rng.standard_normal((M, 256, d // M)) * 20).astype(np.float32)
    o = B.OracleIVFPQ(d, nlist, M, 8, B.METRIC_L2, bucket_init_size=100)   # encodes the base into the lists
    o.set_trained(cc, pq, None)
    B.lib().go_set_assign_mode(0)
    assert o.add(base)
    o.set_raw(base)
    case = dict(d=d, nlist=nlist, M=M, N=N, nq=nq, metric=B.METRIC_L2, base=base, q=q, cc=cc, pq=pq, oracle=o)
    g = fixtures.load_hip(case, bucket_init_size=100)
    try:
        args = api.SearchArgs(metric=api.METRIC_L2, nprobe=16, recall_num=100, has_rank=True, coarse_mode=1, **WIDE)
        g.set_coarse_fused(0)
        D0, I0 = g.ivfpq_search(q, 10, args)
        g.set_coarse_fused(1)
        D1, I1 = g.ivfpq_search(q, 10, args)
        assert g.coarse_filter_stats()["queries"] >= nq
        assert D0.tobytes() == D1.tobytes() and np.array_equal(I0, I1)
    finally:
        g.close()
