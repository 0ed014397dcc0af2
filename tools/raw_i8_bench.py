"""The 8-bit raw stores against the fp32 one, same handle contents, one process ("8-bit raw stores").

  python tools/raw_i8_bench.py --shape c3  [--n 1000000] [--out profiles/raw_i8_c3.json]
  python tools/raw_i8_bench.py --shape emb [--n 500000]

The rows are integer-valued in [0, 127], the values that uint8 AND int8 hold, so one base serves the three stores and the
results of the three must be identical: asserted.
c3 : n x 128, min(rint(synth.sift_like / 2), 127), L2, nlist 4096, M 16, nprobe 32, recall_num 200, k 10, 16384-query device-pointer
     calls.
emb: n x 768, clip(rint(64 + 444 x synth.embedding_like), 0, 127) (a component of a unit vector has sigma 0.036: +-4 sigma fill
     the range), queries synth.embedding_like as they are, inner product, M 64, nprobe 64, recall_num 1000, k 10, 4096-query
     calls.
Per store: queries/s (median of --reps repetitions of --calls calls, min - max), the re-rank stage's us per call
(gamma_hip_profile_get, a pass of its own), single-query p50, the store's bytes.  One JSON line."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from gamma_amd import api, synth


def c3_rows(n, d, seed):
    return np.minimum(np.rint(synth.sift_like(n, d=d, seed=seed) * np.float32(0.5)), np.float32(127.0)).astype(np.float32)


def emb_rows(n, d, seed):
    x = synth.embedding_like(n, d=d, seed=seed)
    return np.clip(np.rint(64.0 + 444.0 * x), 0.0, 127.0).astype(np.float32)


SHAPES = {
    "c3": dict(d=128, nlist=4096, M=16, P=32, R=200, k=10, nq=16384, metric=api.METRIC_L2, rows=c3_rows, queries=c3_rows,
               lo=0.0, hi=1e30),
    "emb": dict(d=768, nlist=4096, M=64, P=64, R=1000, k=10, nq=4096, metric=api.METRIC_IP, rows=emb_rows,
                queries=lambda n, d, seed: synth.embedding_like(n, d=d, seed=seed), lo=-1e30, hi=1e30),
}
DTYPES = ("float32", "uint8", "int8")


def build(S, base, cc, pq, dtype):
    g = api.GammaHip(0)
    g.ivfpq_init(S["d"], S["nlist"], S["M"], 8, S["metric"], bucket_init_size=max(200, int(1.3 * len(base) / S["nlist"])))
    g.ivfpq_set_trained(cc, pq, None)
    g.raw_init(S["d"], dtype)
    for c in range(0, len(base), 250000):
        g.raw_append(base[c:c + 250000])
        g.add(base[c:c + 250000], c)
    return g


def measure(S, g, q, reps, calls):
    dev = torch.device("cuda", 0)
    nq, k = S["nq"], S["k"]
    args = api.SearchArgs(metric=S["metric"], nprobe=S["P"], recall_num=S["R"], has_rank=True, min_score=S["lo"], max_score=S["hi"])
    dq = torch.from_numpy(q).to(dev)
    D = torch.empty((nq, k), dtype=torch.float32, device=dev)
    I = torch.empty((nq, k), dtype=torch.int64, device=dev)
    run = lambda i: g.ivfpq_search_device(dq[(i % 2) * nq:].data_ptr(), nq, k, args, D.data_ptr(), I.data_ptr())
    for i in range(2):
        run(i)
    g.synchronize()
    qps = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for i in range(calls):
            run(i)
        g.synchronize()
        qps.append(nq * calls / (time.perf_counter() - t0))
    rr = []
    g.profile_enable(True)
    for _ in range(reps):
        g.profile_reset()
        for i in range(calls):
            run(i)
        g.synchronize()
        ms, n = g.profile()["rerank"]
        rr.append(1e3 * ms / max(1, n))
    g.profile_enable(False)
    run(0)
    g.synchronize()
    first = (D.cpu().numpy().copy(), I.cpu().numpy().copy())
    lat = []
    for i in range(300):
        t0 = time.perf_counter()
        g.ivfpq_search(q[i:i + 1], k, args)
        lat.append(1e6 * (time.perf_counter() - t0))
    st = g.raw_stats()
    out = dict(qps_median=float(np.median(qps)), qps_min=min(qps), qps_max=max(qps),
               rerank_us_per_call_median=float(np.median(rr)), rerank_us_min=min(rr), rerank_us_max=max(rr),
               single_query_p50_us=float(np.median(lat[50:])), raw_elem_bytes=g.raw_elem_bytes(), raw_elem_type=g.raw_elem_type(),
               raw_store_bytes=st["capacity"] * S["d"] * g.raw_elem_bytes(), raw_rows_bytes=st["rows"] * S["d"] * g.raw_elem_bytes(),
               total_mem_bytes=g.total_mem_bytes())
    return out, first


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), default="c3")
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
    cc, pq = api.train_ivfpq(base[:min(n, S["nlist"] * 40)], S["nlist"], S["M"])
    res = dict(shape=a.shape, n=n, d=S["d"], nlist=S["nlist"], M=S["M"], nprobe=S["P"], recall_num=S["R"], k=S["k"],
               nq_call=S["nq"], calls=a.calls, reps=a.reps, build_s=None)
    firsts = {}
    for dtype in DTYPES:
        g = build(S, base, cc, pq, dtype)
        try:
            res[dtype], firsts[dtype] = measure(S, g, q, a.reps, a.calls)
        finally:
            g.close()
    res["build_s"] = round(time.time() - t0, 1)
    D32, I32 = firsts["float32"]
    same = all(firsts[t][0].tobytes() == D32.tobytes() and firsts[t][1].tobytes() == I32.tobytes() for t in DTYPES[1:])
    res["results_identical"] = bool(same)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    assert same, "the byte stores are lossless: the three stores must give identical results"


if __name__ == "__main__":
    main()
