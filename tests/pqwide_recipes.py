"""Inputs of the wide-PQ edge and fuzz tests (tests/test_gpu_pqwide_edges.py, tests/test_gpu_pqwide_fuzz.py), built from the CPU
oracle alone so that tests/test_pqwide_recipes_cpu.py can assert, without a GPU, that they are what the GPU tests claim: the
list lengths, the unit count of the list-major scan, the sub-batches a workspace budget cuts a call into, the rows that still
hold k results under a filter or a window, and what the default fuzz seeds cover.

Nothing is trained here: coarse centroids and PQ codebooks are samples of the data (exact parity does not need good ones)."""
import os

import numpy as np

from gamma_amd import synth
from oracle import binding as B

WIDE = dict(min_score=-3e38, max_score=3e38)
# pqwide_lm.hip WIDE_LM_GRID; kernels.h kWideLmSlab, kWideLmQueryTile; gamma_hip_search.cpp kWideTableBytes
LM_GRID, LM_SLAB, LM_QT = 512, 256, 8
WIDE_TABLE_BYTES = 1 << 30
BIG_BUDGET = 8 << 30


def sampled_state(base, nlist, M, rng):
    """coarse centroids = sampled rows, a few entries nudged so that no two are equal -- by a power of two near 1 / 512 of the
    data's largest entry (0.25 on SIFT-shaped rows), so normalised rows keep centroids of about unit norm and grid data stays
    exact; codebooks = 256 sampled sub-vectors per sub-quantizer"""
    N, d = base.shape
    dsub = d // M
    nudge = np.float32(2.0 ** np.floor(np.log2(max(float(np.abs(base).max()), 1e-30) / 512.0)))
    cc = base[rng.choice(N, nlist, replace=False)] + (rng.random((nlist, d)) < 0.05).astype(np.float32) * nudge
    pq = np.stack([base[rng.choice(N, 256, replace=N < 256), m * dsub:(m + 1) * dsub] for m in range(M)])
    return np.ascontiguousarray(cc, np.float32), np.ascontiguousarray(pq, np.float32)


def bitmap_of(docs, nbits):
    bm = np.zeros((nbits >> 3) + 1, dtype=np.uint8)
    docs = np.asarray(docs, dtype=np.int64)
    np.bitwise_or.at(bm, docs >> 3, (1 << (docs & 7)).astype(np.uint8))
    return bm


def oracle_search(o, q, call, filt=None):
    """call: dict(k, P, R, metric, has_rank); filt: None or dict(bitmap, docs, not_in, lo, hi) -- (D, I, stages)"""
    f = filt or {}
    rf = [B.make_range_filter(f["docs"], b_not_in=f.get("not_in", False))] if f.get("docs") is not None else None
    ctx = B.make_ctx(docids_bitmap=f.get("bitmap"), range_filters=rf, min_score=f.get("lo", -3e38), max_score=f.get("hi", 3e38))
    return o.search(q, call["k"], call["P"], recall_num=call["R"], has_rank=call["has_rank"], metric=call["metric"], ctx=ctx,
                    want_stages=True)


def full_rows(I):
    """queries whose k results are all there"""
    return int((np.asarray(I)[:, -1] != -1).sum())


def window_of(D, I):
    """a score window from the oracle's unrestricted distances: the 5 % quantile of the rows' lowest and the 95 % quantile of
    their highest value, over the rows that hold k results -- about a tenth of the queries lose an end of their row"""
    rows = np.asarray(I)[:, -1] != -1
    if not rows.any():
        return -3e38, 3e38
    D = np.asarray(D)[rows]
    return float(np.quantile(D.min(axis=1), 0.05)), float(np.quantile(D.max(axis=1), 0.95))


# ---- 1a: lists at the kernels' boundaries -----------------------------------------------------------------------------------
EDGE_LENS = [0, 1, 255, 256, 257, 511, 512, 513, 1025, 0, 64, 63]
EDGE_M = (65, 96, 256)
EDGE_VARIANTS = ("plain", "filter_in", "filter_not_in", "window")
_edge = {}


def edge_fill(o, st):
    """the lists of an edge state into an oracle made by the caller (the mode-0 one is made under a lowered table limit)"""
    o.set_trained(st["cc"], st["pq"], None)
    o.set_raw(st["base"])
    for l, keys in enumerate(st["keys"]):
        if len(keys):
            assert o.add_keys(l, keys, st["codes"][keys])
    return o


def edge_state(M):
    """12 lists of EDGE_LENS codes over 3457 SIFT-shaped rows of d = 2 M; every row's code is the oracle's encoding of it,
    the list it sits in is dealt by a permutation (any placement has a defined answer).  64 queries near the centroids:
    eight per list of 255 codes and more, two per empty list and per one-code list, one per list of 64 and of 63 -- so at
    nprobe 1 the short lists are probed and seven queries in eight can still fill k = 50 under the filter."""
    if M in _edge:
        return _edge[M]
    rng = np.random.default_rng(4100 + M)
    d, nlist, N = 2 * M, len(EDGE_LENS), sum(EDGE_LENS)
    base = synth.sift_like(N, d=d, seed=4200 + M)
    cc, pq = sampled_state(base, nlist, M, rng)
    perm, keys, at = rng.permutation(N), [], 0
    for n in EDGE_LENS:
        keys.append(np.sort(perm[at:at + n]).astype(np.int64))
        at += n
    targets = np.array([l for l in (2, 3, 4, 5, 6, 7, 8) for _ in range(8)] + [0, 0, 1, 1, 9, 9, 10, 11])
    q = (np.float32(0.9) * cc[targets] + np.float32(0.1) * base[rng.integers(0, N, len(targets))]).astype(np.float32)
    st = dict(M=M, d=d, nlist=nlist, N=N, base=base, cc=cc, pq=pq, keys=keys, q=q, targets=targets, metric=B.METRIC_L2)
    # 1000 queries spread over all centroids: at nprobe 12 the pair scan takes two probes per workgroup (scan_group_size), and
    # an inner-product segment of an empty list and a list of at most one tile keeps its sums in registers past the skipped probe
    st["q_big"] = (np.float32(0.9) * cc[rng.integers(0, nlist, 1000)] + np.float32(0.1) * base[rng.integers(0, N, 1000)]).astype(np.float32)
    o = B.OracleIVFPQ(d, nlist, M, 8, B.METRIC_L2)
    o.set_trained(cc, pq, None)
    st["codes"] = o.encode(base)[1]
    st["oracle"] = edge_fill(o, st)
    st["deleted"] = rng.choice(N, N // 5, replace=False)   # 20 %
    st["bitmap"] = bitmap_of(st["deleted"], N)
    st["docs"] = rng.choice(N, N // 2, replace=False)
    _edge[M] = st
    return st


def edge_calls():
    calls = [dict(nq=64, P=P, metric=metric, has_rank=has_rank, k=k, R=R)
             for P in (1, 12) for metric in (B.METRIC_L2, B.METRIC_IP) for has_rank in (True, False)
             for k, R in ((1, 1), (10, 5), (10, 50), (50, 300))]
    calls += [dict(nq=nq, P=12, metric=metric, has_rank=True, k=10, R=50) for nq in (1, 3) for metric in (B.METRIC_L2, B.METRIC_IP)]
    return calls


EDGE_BIG_CALL = dict(nq=1000, P=12, metric=B.METRIC_IP, has_rank=True, k=10, R=50)   # (the plain variant only)


def scan_group_size(nq, P, G0=8):
    """probes per workgroup of the pair scan (scan_plan.cpp scan_group_size; G0 = 8 for lists of at most 700 codes on average and
    nprobe <= 64): halved until nq x the groups per query reach 4096 workgroups"""
    G = G0
    while G > 1 and nq * -(-P // G) < 4096:
        G >>= 1
    return max(1, min(G, P))


def edge_filter(st, variant, call):
    """the filter of a call under a variant; the window comes from the mode-1 oracle's unrestricted answer to the call's
    parameters over all 64 queries (quantiles of the one or three rows of a small call say nothing)"""
    if variant == "plain":
        return None
    if variant == "window":
        D, I, _ = oracle_search(st["oracle"], st["q"], call)
        lo, hi = window_of(D, I)
        return dict(lo=lo, hi=hi)
    return dict(bitmap=st["bitmap"], docs=st["docs"], not_in=variant == "filter_not_in")


# ---- 1b: more units than the list-major grid ----------------------------------------------------------------------------------
def lm_units(lens, probes):
    """work units of k_ivfpq_scan_wide_lm: per probed, non-empty list, slabs of 256 codes x tiles of 8 (query, probe) pairs"""
    lens = np.asarray(lens, dtype=np.int64)
    pairs = np.bincount(np.asarray(probes).ravel(), minlength=len(lens)).astype(np.int64)
    return int((-(-lens // LM_SLAB) * -(-pairs // LM_QT))[(lens > 0)].sum())


def units_case(nq=1000):
    from tests import fixtures
    case = fixtures.trained_case(192, nlist=8, M=96, N=5000, nq=64)
    q = synth.sift_like(nq, d=192, seed=1700 + nq)
    return case, q


def list_lens(o, nlist):
    return [o.list_size(l) for l in range(nlist)]


# ---- 1c: several sub-batches per call -------------------------------------------------------------------------------------------
def scan_chunk(budget, lens, probes, M, table_limited=True):
    """queries per sub-batch of a wide call, as ivfpq_search_device_locked sizes them: by nprobe x the longest list first and,
    when that cuts the call, by the batch's longest candidate row measured on the device (rounded up to 4); a call whose
    tables are built ahead of the scan is limited to 1 GB of them as well (table_limited: all but L2 in table mode 0)"""
    nq, P = probes.shape
    lens = np.asarray(lens, dtype=np.int64)
    wide = max(1, WIDE_TABLE_BYTES // (M * 1024)) if table_limited else 1 << 62
    chunk = max(1, min(budget // (P * max(1, int(lens.max())) * 4), wide, nq))
    if chunk < nq:
        cap = (max(int(lens[probes].sum(axis=1).max()), 1) + 3) & ~3
        chunk = max(chunk, min(budget // (cap * 4), wide, nq))
    return int(chunk)


def ties_case():
    """tests/test_gpu_pqwide.py::test_exact_ties_at_the_recall_cut's data (200 rows four times each) with 300 queries"""
    from tests import fixtures
    case = fixtures.trained_case(192, nlist=8, M=96, N=5000, nq=64)
    base = synth.sift_like(2200, d=192, seed=77)
    base = np.concatenate([base, np.repeat(base[:200], 3, axis=0)])
    q = base[:300] + np.float32(0.25)
    return case, base, q


def ties_oracle(case, base):
    o = B.OracleIVFPQ(192, 8, 96, 8, B.METRIC_L2)
    o.set_trained(case["cc"], case["pq"], None)
    B.lib().go_set_assign_mode(0)
    assert o.add(base)
    o.set_raw(base)
    return o


def ties_budget(lens, P):
    """room for the slab of 37 queries at the general stride (nprobe x the longest list)"""
    return 37 * P * max(1, max(lens)) * 4


# ---- 1d: an inner-product index -------------------------------------------------------------------------------------------------
def ip_case(M):
    """3000 normalised SIFT-shaped rows of d = 2 M under an index created with METRIC_IP, 8 lists, 64 normalised queries"""
    rng = np.random.default_rng(4300 + M)
    d, nlist, N = 2 * M, 8, 3000
    unit = lambda x: (x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-9)).astype(np.float32)
    base, q = unit(synth.sift_like(N, d=d, seed=4400 + M)), unit(synth.sift_like(64, d=d, seed=4500 + M))
    cc, pq = sampled_state(base, nlist, M, rng)
    o = B.OracleIVFPQ(d, nlist, M, 8, B.METRIC_IP)
    o.set_trained(cc, pq, None)
    B.lib().go_set_assign_mode(0)
    assert o.add(base)
    o.set_raw(base)
    return dict(d=d, nlist=nlist, M=M, metric=B.METRIC_IP, cc=cc, pq=pq, base=base, q=q, oracle=o)


# ---- 2: the fuzz ----------------------------------------------------------------------------------------------------------------
FUZZ_DEFAULT_SEEDS = [1, 2, 3, 4, 6, 7, 8, 11]
FUZZ_SEEDS = [int(s) for s in os.environ.get("GAMMA_PQWIDE_FUZZ_SEEDS", ",".join(map(str, FUZZ_DEFAULT_SEEDS))).split(",")
              if s.strip()]


def fuzz_plan(seed):
    """everything a seed decides, without the data"""
    rng = np.random.default_rng(260000 + seed)
    M = int(rng.choice([65, 66, 80, 95, 96, 97, 127, 128, 160, 192, 200, 224, 255, 256]))
    dsub = int(rng.choice([x for x in (1, 2, 3, 4, 8) if x * M <= 1040]))
    nlist = int(rng.choice([5, 9, 16]))
    N = int(rng.integers(600, 4001))
    p = dict(seed=seed, M=M, dsub=dsub, d=M * dsub, nlist=nlist, N=N, kind=str(rng.choice(["sift", "grid3", "grid8"])),
             ip_index=bool(rng.integers(0, 2)), bucket=int(rng.choice([50, 1000])))
    # now and then a centroid far from the data: its list stays empty and is probed when nprobe = nlist
    p["far"] = int(rng.integers(0, nlist)) if rng.random() < 0.4 else -1
    p["batches"], at = [], 0
    while at < N:   # fewer than 20 vectors take the exact assignment
        n = int(min(N - at, rng.choice([5, 19, 20, 333, 1000])))
        p["batches"].append(n)
        at += n
    p["ndel"] = int(rng.integers(0, N // 4 + 1))
    p["nupd"] = int(rng.integers(1, 7))
    p["compact"] = bool(rng.integers(0, 2))
    p["searches"] = []
    for i in range(4):
        s = dict(nq=int(rng.choice([1, 3, 19, 20, 64, 300])), k=int(rng.choice([1, 5, 10, 33])),
                 R=int(rng.choice([1, 7, 40, 100, 300])), P=int(rng.integers(1, nlist + 1)),
                 metric=B.METRIC_L2 if rng.integers(0, 2) else B.METRIC_IP, has_rank=bool(rng.integers(0, 2)),
                 ranged=bool(rng.random() < 0.35), not_in=bool(rng.integers(0, 2)), frac=float(rng.choice([0.3, 0.7])),
                 reduced=bool(rng.random() < 0.3))
        if i == 0 and p["far"] >= 0:
            s["P"] = nlist
        p["searches"].append(s)
    return p


def _fuzz_rows(kind, n, d, seed, rng):
    if kind == "sift":
        return synth.sift_like(n, d=d, seed=seed)
    return rng.integers(0, 3 if kind == "grid3" else 8, size=(n, d)).astype(np.float32)


def fuzz_data(p):
    rng = np.random.default_rng(270000 + p["seed"])
    N, d, nlist, M = p["N"], p["d"], p["nlist"], p["M"]
    base = _fuzz_rows(p["kind"], N, d, 2600 + p["seed"], rng)
    if p["ip_index"] and p["kind"] == "sift":
        base = (base / np.maximum(np.linalg.norm(base, axis=1, keepdims=True), 1e-9)).astype(np.float32)
    cc, pq = sampled_state(base, nlist, M, rng)
    if p["far"] >= 0:
        cc[p["far"]] += np.float32(1000.0)
    dt = dict(p, base=base, cc=cc, pq=pq, metric=B.METRIC_IP if p["ip_index"] else B.METRIC_L2)
    dt["queries"], dt["docs"] = [], []
    for i, s in enumerate(p["searches"]):
        nq = s["nq"]
        fresh = _fuzz_rows(p["kind"], nq - nq // 2, d, 2700 + 10 * p["seed"] + i, rng)
        if p["ip_index"] and p["kind"] == "sift":
            fresh = (fresh / np.maximum(np.linalg.norm(fresh, axis=1, keepdims=True), 1e-9)).astype(np.float32)
        dt["queries"].append(np.ascontiguousarray(np.concatenate([base[rng.integers(0, N, nq // 2)], fresh]), np.float32))
        dt["docs"].append(rng.choice(N, max(1, int(N * s["frac"])), replace=False) if s["ranged"] else None)
    return dt


def fuzz_oracle_add(o, dt):
    """the Add path in the plan's batches (faiss's rule: fewer than 20 vectors exact, else the GEMM form); the caller sets and
    restores go_set_assign_mode; returns the oracle's delete bitmap (consulted by its list writer, so each oracle has its own)"""
    o.set_trained(dt["cc"], dt["pq"], None)
    o.set_raw(dt["base"])
    bm = np.zeros((dt["N"] + 64) // 8 + 1, dtype=np.uint8)
    o.set_docids_bitmap(bm)
    at = 0
    for n in dt["batches"]:
        assert o.add(dt["base"][at:at + n])
        at += n
    return bm


def fuzz_edits(o, dt):
    """the documents to delete and the entries to update, decided once the lists exist (dt["dead"], dt["updates"]): up to
    ndel documents anywhere and -- on a compacting seed -- 40 % of the entries of up to two lists of 20 codes and more, so
    that CompactIfNeed (a list is rewritten from 30 % of deleted entries on) has lists to rewrite; never more than a quarter
    of the documents in all"""
    rng = np.random.default_rng(280000 + dt["seed"])
    N, nlist = dt["N"], dt["nlist"]
    budget, dead = N // 4, np.zeros(0, np.int64)
    if dt["compact"]:
        taken = 0
        for l in rng.permutation(nlist):
            ids = o.get_list(int(l))[0]
            need = -(-2 * len(ids) // 5)
            if len(ids) >= 20 and len(dead) + need <= budget and taken < 2:
                dead = np.concatenate([dead, rng.choice(ids, need, replace=False)])
                taken += 1
    rest = np.setdiff1d(np.arange(N), dead)
    dead = np.concatenate([dead, rng.choice(rest, min(dt["ndel"], budget - len(dead)), replace=False)]).astype(np.int64)
    live = np.setdiff1d(np.arange(N), dead)
    others = [l for l in range(nlist) if l != dt["far"]]
    dt["dead"] = dead
    dt["updates"] = [(int(rng.choice(others)), int(v), rng.integers(0, 256, size=dt["M"]).astype(np.uint8))
                     for v in rng.choice(live, min(dt["nupd"], len(live)), replace=False)]


def fuzz_oracle_edit(o, bm, dt):
    """Delete, Update and -- on some seeds -- CompactIfNeed (dt["dead"], dt["updates"]: fuzz_edits); returns the list lengths
    as they stood before the compaction"""
    dead = dt["dead"]
    if len(dead):
        np.bitwise_or.at(bm, dead >> 3, (1 << (dead & 7)).astype(np.uint8))
        o.delete(dead)
    for newl, vid, code in dt["updates"]:
        o.update_code(newl, vid, code)
    before = list_lens(o, dt["nlist"])
    if dt["compact"]:
        o.compact_if_need(bm)
    return before


def fuzz_oracle(dt):
    o = B.OracleIVFPQ(dt["d"], dt["nlist"], dt["M"], 8, dt["metric"], bucket_init_size=dt["bucket"])
    B.lib().go_set_assign_mode(-1)
    try:
        bm = fuzz_oracle_add(o, dt)
    finally:
        B.lib().go_set_assign_mode(0)
    fuzz_edits(o, dt)
    dt["lens_before_compaction"] = fuzz_oracle_edit(o, bm, dt)
    return o, bm


def fuzz_filter(dt, i, bm):
    s = dt["searches"][i]
    return dict(bitmap=bm, docs=dt["docs"][i], not_in=s["not_in"])


def fuzz_budget(P, max_len):
    return max(1 << 16, 50 * P * max(1, max_len) * 4)
