"""Flat search over a scalar-quantised (sq8) store against the fp32 and the float16 store, one process.

  timeout -k 10 600 python tools/flat_sq8_bench.py --shape c2  [--n 1000000] [--out profiles/flat_sq8_c2.json]
  timeout -k 10 900 python tools/flat_sq8_bench.py --shape emb [--n 1000000] [--out profiles/flat_sq8_emb.json]

(each shape is a run of its own under a time limit of its own).  The base is float data: c2 = synth.sift_like, n x 128, L2;
emb = synth.embedding_like, n x 768, inner product; k 100, 1024-query device-pointer calls.  Three stores are built in the one
process:
  sq8     : the base, ranges trained on its first 100000 rows (the rest clips where it reaches beyond them)
  float32 : W = decode(encode(base)) with those ranges (tests/sq8_ref.py) -- the rows the sq8 store holds.  THE YARDSTICK: the
            results of the two must be identical (asserted), so the two calls do the same job
  float16 : the base rounded to binary16 -- the other store float data can use, half the bytes, other rows (no identity)
Per store: ms per call (median of --reps repetitions of --calls calls, min - max), queries/s, the store's bytes.  For sq8 and
float16 the ratio of medians against float32 and whether the median lies inside the float32 repetitions' own min - max spread or
below it ("not slower").  A reported figure, not a gate.  One JSON line."""
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

SHAPES = {
    "c2": dict(d=128, k=100, nq=1024, metric=api.METRIC_L2, rows=lambda n, d, seed: synth.sift_like(n, d=d, seed=seed)),
    "emb": dict(d=768, k=100, nq=1024, metric=api.METRIC_IP, rows=lambda n, d, seed: synth.embedding_like(n, d=d, seed=seed)),
}
STORES = ("float32", "float16", "sq8")
CHUNK = 250000


def build(S, dtype, base, train):
    """(handle, ranges or None)"""
    g = api.GammaHip(0)
    g.raw_init(S["d"], dtype)
    ranges = None
    if dtype == "sq8":
        g.raw_sq8_train(train)
        ranges = g.raw_sq8_get_ranges()
        g.set_flat_sq8_rows(True)
    elif dtype != "float32":
        g.set_flat_narrow_rows(True)
    for c in range(0, len(base), CHUNK):
        g.raw_append(base[c:c + CHUNK])
    return g, ranges


def measure(S, g, q, reps, calls):
    dev = torch.device("cuda", 0)
    nq, k = S["nq"], S["k"]
    args = api.SearchArgs(metric=S["metric"], min_score=-3e38, max_score=3e38)
    dq = torch.from_numpy(q).to(dev)
    D = torch.empty((nq, k), dtype=torch.float32, device=dev)
    I = torch.empty((nq, k), dtype=torch.int64, device=dev)
    run = lambda i: g.flat_search_device(dq[(i % 2) * nq:].data_ptr(), nq, k, args, D.data_ptr(), I.data_ptr())
    for i in range(2):
        run(i)
    g.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for i in range(calls):
            run(i)
        g.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0) / calls)
    run(0)
    g.synchronize()
    first = (D.cpu().numpy().copy(), I.cpu().numpy().copy())
    st = g.raw_stats()
    med = float(np.median(ms))
    out = dict(ms_per_call_median=med, ms_min=min(ms), ms_max=max(ms), qps_median=nq / med * 1e3, raw_elem_bytes=g.raw_elem_bytes(),
               raw_elem_type=g.raw_elem_type(), raw_rows_bytes=st["rows"] * S["d"] * g.raw_elem_bytes(),
               total_mem_bytes=g.total_mem_bytes(), flat_filter_stats=list(g.flat_filter_stats()))
    return out, first


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), default="c2")
    ap.add_argument("--n", type=float, default=1e6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    S = SHAPES[a.shape]
    n, d = int(a.n), S["d"]
    t0 = time.time()
    base = S["rows"](n, d, 1234)
    q = S["rows"](2 * S["nq"], d, 4321)
    train = base[:min(n, 100000)]
    res = dict(shape=a.shape, n=n, d=d, k=S["k"], nq_call=S["nq"], metric="L2" if S["metric"] == api.METRIC_L2 else "IP",
               calls=a.calls, reps=a.reps, build_s=None)
    firsts = {}
    # sq8 first: its trained ranges define W, the rows of the fp32 yardstick
    g, (vmin, vmax) = build(S, "sq8", base, train)
    try:
        res["sq8"], firsts["sq8"] = measure(S, g, q, a.reps, a.calls)
    finally:
        g.close()
    step, inv = sq8_ref.params(vmin, vmax)
    codes = np.empty((n, d), np.uint8)
    W = np.empty((n, d), np.float32)
    for c in range(0, n, CHUNK):
        codes[c:c + CHUNK] = sq8_ref.encode(base[c:c + CHUNK], vmin, inv)
        W[c:c + CHUNK] = sq8_ref.decode(codes[c:c + CHUNK], vmin, step)
    res["sq8"]["clipped_values"] = int(((base < vmin) | (base > vmax)).sum())
    del codes
    for dtype, rows in (("float32", W), ("float16", base)):
        g, _ = build(S, dtype, rows, None)
        try:
            res[dtype], firsts[dtype] = measure(S, g, q, a.reps, a.calls)
        finally:
            g.close()
    res["build_s"] = round(time.time() - t0, 1)
    f32 = res["float32"]
    for t in ("float16", "sq8"):
        res[t]["ms_vs_float32"] = res[t]["ms_per_call_median"] / f32["ms_per_call_median"]
        res[t]["not_slower_than_float32_spread"] = bool(res[t]["ms_per_call_median"] <= f32["ms_max"])
    same = firsts["sq8"][0].tobytes() == firsts["float32"][0].tobytes() and firsts["sq8"][1].tobytes() == firsts["float32"][1].tobytes()
    res["sq8_results_identical_to_float32_of_W"] = bool(same)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    assert same, "the sq8 store and the fp32 store of the decoded rows must give identical results"


if __name__ == "__main__":
    main()
