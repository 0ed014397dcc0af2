"""IVFFLAT search over a scalar-quantised (sq8) store against the fp32 and the float16 store: same lists, one process (DESIGN.md
section 25).

  timeout -k 10 900 python tools/ivfflat_sq8_bench.py [--shape lm|pair|emb|all] [--out profiles/ivfflat_sq8_{shape}.json]

lm  : 1 M x 128 synth.sift_like, nlist 4096, nprobe 32, k 10, L2 (the README's IVFFLAT shape), 4096-query device-pointer calls --
      the list-major kernel (k_ivfflat_lm).
pair: the same index, 64-query calls -- the small path, one workgroup per (query, probe) pair (k_ivfflat_scan).
emb : 500 k x 768 synth.embedding_like, inner product, nlist 1024, nprobe 32, k 10, 4096-query calls -- the row-sliced list-major
      kernel (k_ivfflat_lms).
Three handles per index, built in the one process:
  sq8     : the base, ranges trained on its first 100000 rows (the rest clips where it reaches beyond them).  It assigns the
            vectors -- coarse assignment sees the caller's fp32 rows -- and the other two get its lists.
  float32 : W = decode(encode(base)) with those ranges (tests/sq8_ref.py) -- the rows the sq8 store holds.  THE YARDSTICK: the
            results of the two must be identical (asserted), so the two calls do the same job.
  float16 : the base rounded to binary16 -- the other store float data can use, half the bytes, other rows (no identity).
Per store: ms per call (median of --reps repetitions of --calls calls, min - max), queries/s, the store's bytes, the path counters
of the measured calls.  For sq8 and float16 the ratio of medians against float32 and whether the median lies inside the float32
repetitions' own min - max spread or below it ("not slower").  A reported figure, not a gate.  One JSON line per shape."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from gamma_amd import api, synth
from tests import sq8_ref

K, NPROBE = 10, 32
INDEXES = {
    "sift": dict(n=1000000, d=128, nlist=4096, metric=api.METRIC_L2, rows=lambda n, d, seed: synth.sift_like(n, d=d, seed=seed)),
    "emb": dict(n=500000, d=768, nlist=1024, metric=api.METRIC_IP, rows=lambda n, d, seed: synth.embedding_like(n, d=d, seed=seed)),
}
SHAPES = {"lm": ("sift", 4096), "pair": ("sift", 64), "emb": ("emb", 4096)}
STORES = ("float32", "float16", "sq8")
CHUNK = 1 << 16


def build(X, cc, dtype, rows, lists, train=None):
    """lists: None -- the handle assigns the vectors itself; else (list numbers, counts, vids) of the handle that did"""
    g = api.GammaHip(0)
    g.ivfflat_init(X["d"], X["nlist"], X["metric"], bucket_init_size=max(1000, int(2.5 * len(rows) / X["nlist"])))
    g.ivfflat_set_trained(cc)
    g.raw_init(X["d"], dtype)
    if dtype == "sq8":
        g.raw_sq8_train(train)
        g.set_ivfflat_sq8_rows(True)
    elif dtype != "float32":
        g.set_ivfflat_narrow_rows(True)
    for c in range(0, len(rows), CHUNK):
        xb = rows[c:c + CHUNK]
        g.raw_append(xb)
        if lists is None:
            g.add(xb, c)
    if lists is not None:
        g.add_keys_batch(lists[0], lists[1], lists[2], np.zeros((len(lists[2]), 1), np.uint8))
    return g


def lists_of(g, nlist):
    nos, counts, vids = [], [], []
    for l in range(nlist):
        ids = g.get_list(l)[0]
        if len(ids):
            nos.append(l)
            counts.append(len(ids))
            vids.append(ids)
    return nos, counts, np.concatenate(vids)


def measure(X, g, q, nq, reps, calls):
    dev = torch.device("cuda", 0)
    args = api.SearchArgs(metric=X["metric"], nprobe=NPROBE, min_score=-3e38, max_score=3e38)
    dq = torch.from_numpy(q).to(dev)
    Dd = torch.empty((nq, K), dtype=torch.float32, device=dev)
    Id = torch.empty((nq, K), dtype=torch.int64, device=dev)
    run = lambda i: g.ivfflat_search_device(dq[(i % 2) * nq:].data_ptr(), nq, K, args, Dd.data_ptr(), Id.data_ptr())
    for i in range(2):
        run(i)
    g.synchronize()
    g.ivfflat_scan_stats(reset=True)
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for i in range(calls):
            run(i)
        g.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0) / calls)
    stats = list(g.ivfflat_scan_stats())
    run(0)
    g.synchronize()
    first = (Dd.cpu().numpy().copy(), Id.cpu().numpy().copy())
    st = g.raw_stats()
    med = float(np.median(ms))
    out = dict(ms_per_call_median=med, ms_min=min(ms), ms_max=max(ms), qps_median=nq / med * 1e3, raw_elem_bytes=g.raw_elem_bytes(),
               raw_elem_type=g.raw_elem_type(), raw_rows_bytes=st["rows"] * X["d"] * g.raw_elem_bytes(),
               total_mem_bytes=g.total_mem_bytes(), scan_stats_small_pair_lm_lms=stats)
    return out, first


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES) + ["all"], default="all")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--out", default="", help="file of the JSON line; {shape} is replaced")
    a = ap.parse_args()
    shapes = ["lm", "pair", "emb"] if a.shape == "all" else [a.shape]
    ok = True
    for name in ("sift", "emb"):
        mine = [s for s in shapes if SHAPES[s][0] == name]
        if not mine:
            continue
        X = INDEXES[name]
        n, d, nlist = X["n"], X["d"], X["nlist"]
        t0 = time.time()
        base = X["rows"](n, d, 1234)
        q = X["rows"](2 * 4096, d, 4321)
        cc, _ = api.train_ivfpq(base[:nlist * 64], nlist, 16)
        handles = {}
        try:
            # sq8 first: its trained ranges define W, the rows of the fp32 yardstick, and it assigns the caller's rows
            handles["sq8"] = build(X, cc, "sq8", base, None, train=base[:min(n, 100000)])
            vmin, vmax = handles["sq8"].raw_sq8_get_ranges()
            lists = lists_of(handles["sq8"], nlist)
            step, inv = sq8_ref.params(vmin, vmax)
            W = np.empty((n, d), np.float32)
            for c in range(0, n, CHUNK):
                W[c:c + CHUNK] = sq8_ref.decode(sq8_ref.encode(base[c:c + CHUNK], vmin, inv), vmin, step)
            clipped = int(((base < vmin) | (base > vmax)).sum())
            handles["float32"] = build(X, cc, "float32", W, lists)
            del W
            handles["float16"] = build(X, cc, "float16", base, lists)
            build_s = round(time.time() - t0, 1)
            for shape in mine:
                nq = SHAPES[shape][1]
                res = dict(shape=shape, n=n, d=d, nlist=nlist, nprobe=NPROBE, k=K, nq_call=nq,
                           metric="L2" if X["metric"] == api.METRIC_L2 else "IP", calls=a.calls, reps=a.reps, build_s=build_s)
                firsts = {}
                for dtype in STORES:
                    res[dtype], firsts[dtype] = measure(X, handles[dtype], q[:2 * nq], nq, a.reps, a.calls)
                res["sq8"]["clipped_values"] = clipped
                f32 = res["float32"]
                for t in ("float16", "sq8"):
                    res[t]["ms_vs_float32"] = res[t]["ms_per_call_median"] / f32["ms_per_call_median"]
                    res[t]["not_slower_than_float32_spread"] = bool(res[t]["ms_per_call_median"] <= f32["ms_max"])
                same = (firsts["sq8"][0].tobytes() == firsts["float32"][0].tobytes() and
                        firsts["sq8"][1].tobytes() == firsts["float32"][1].tobytes())
                res["sq8_results_identical_to_float32_of_W"] = bool(same)
                ok = ok and same
                line = json.dumps(res)
                print(line, flush=True)
                if a.out:
                    with open(a.out.replace("{shape}", shape), "w") as f:
                        f.write(line + "\n")
        finally:
            for g in handles.values():
                g.close()
    assert ok, "the sq8 store and the fp32 store of the decoded rows must give identical results"


if __name__ == "__main__":
    main()
