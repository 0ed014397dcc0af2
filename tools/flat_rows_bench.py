"""Flat search over float16 / uint8 / int8 rows against the fp32 store, same store contents, one process.

  python tools/flat_rows_bench.py --shape c2  [--n 1000000] [--out profiles/flat_rows_c2.json]
  python tools/flat_rows_bench.py --shape emb [--n 1000000] [--out profiles/flat_rows_emb.json]

The rows are integer-valued in [0, 127], the values that float16, uint8 AND int8 hold, so one base serves the four stores and
the results of the four must be identical: asserted.
c2 : n x 128, min(rint(synth.sift_like / 2), 127), L2, k 100, 1024-query device-pointer calls.
emb: n x 768, clip(rint(64 + 444 x synth.embedding_like), 0, 127), queries synth.embedding_like as they are, inner product,
     k 100, 1024-query calls.
Per store: ms per call (median of --reps repetitions of --calls calls, min - max), queries/s, the store's bytes.  The yardstick is
the fp32 store of the same process: per narrow type the ratio of medians and whether the narrow median lies inside the fp32
repetitions' own min - max spread or below it ("not slower").  One JSON line."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from gamma_amd import api, synth


def c2_rows(n, d, seed):
    return np.minimum(np.rint(synth.sift_like(n, d=d, seed=seed) * np.float32(0.5)), np.float32(127.0)).astype(np.float32)


def emb_rows(n, d, seed):
    x = synth.embedding_like(n, d=d, seed=seed)
    return np.clip(np.rint(64.0 + 444.0 * x), 0.0, 127.0).astype(np.float32)


SHAPES = {
    "c2": dict(d=128, k=100, nq=1024, metric=api.METRIC_L2, rows=c2_rows, queries=c2_rows),
    "emb": dict(d=768, k=100, nq=1024, metric=api.METRIC_IP, rows=emb_rows,
                queries=lambda n, d, seed: synth.embedding_like(n, d=d, seed=seed)),
}
DTYPES = ("float32", "float16", "uint8", "int8")


def build(S, base, dtype):
    g = api.GammaHip(0)
    g.raw_init(S["d"], dtype)
    if dtype != "float32":
        g.set_flat_narrow_rows(True)
    for c in range(0, len(base), 250000):
        g.raw_append(base[c:c + 250000])
    return g


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
               total_mem_bytes=g.total_mem_bytes())
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
    n = int(a.n)
    t0 = time.time()
    base = S["rows"](n, S["d"], 1234)
    q = S["queries"](2 * S["nq"], S["d"], 4321)
    res = dict(shape=a.shape, n=n, d=S["d"], k=S["k"], nq_call=S["nq"], metric="L2" if S["metric"] == api.METRIC_L2 else "IP",
               calls=a.calls, reps=a.reps, build_s=None)
    firsts = {}
    for dtype in DTYPES:
        g = build(S, base, dtype)
        try:
            res[dtype], firsts[dtype] = measure(S, g, q, a.reps, a.calls)
        finally:
            g.close()
    res["build_s"] = round(time.time() - t0, 1)
    f32 = res["float32"]
    for t in DTYPES[1:]:
        res[t]["ms_vs_float32"] = res[t]["ms_per_call_median"] / f32["ms_per_call_median"]
        res[t]["not_slower_than_float32_spread"] = bool(res[t]["ms_per_call_median"] <= f32["ms_max"])
    D32, I32 = firsts["float32"]
    same = all(firsts[t][0].tobytes() == D32.tobytes() and firsts[t][1].tobytes() == I32.tobytes() for t in DTYPES[1:])
    res["results_identical"] = bool(same)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    assert same, "narrow rows widen exactly: the four stores must give identical results"


if __name__ == "__main__":
    main()
