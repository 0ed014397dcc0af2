"""The scalar-quantised raw store against the fp32 and the float16 one, same handle contents, one process (DESIGN.md,
"scalar-quantised raw store").

  python tools/raw_sq8_bench.py --shape c3  [--n 1000000] [--out profiles/raw_sq8_c3.json]
  python tools/raw_sq8_bench.py --shape emb [--n 500000]

The rows are float data (nothing here is integer-valued on purpose), so the byte stores of tools/raw_i8_bench.py cannot hold them.
The sq8 store's ranges are the per-dimension minimum and maximum of the rows the quantizers are trained on, as the HIPIVFPQ model
trains them.
c3 : n x 128, synth.sift_like + uniform noise in [0, 1) (real-valued), L2, nlist 4096, M 16, nprobe 32, recall_num 200, k 10,
     16384-query device-pointer calls.
emb: n x 768, synth.embedding_like (unit-normalised), inner product, M 64, nprobe 64, recall_num 1000, k 10, 4096-query calls.
Per store: queries/s (median of --reps repetitions of --calls calls, min - max), the re-rank stage's us per call
(gamma_hip_profile_get, a pass of its own), single-query p50, the store's bytes, and recall@10 of 1024 queries against flat
search over the fp32 rows.  One JSON line."""
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
    noise = np.random.default_rng(seed + 99).random((n, d), dtype=np.float32)
    return (synth.sift_like(n, d=d, seed=seed) + noise).astype(np.float32)


def emb_rows(n, d, seed):
    return synth.embedding_like(n, d=d, seed=seed)


SHAPES = {
    "c3": dict(d=128, nlist=4096, M=16, P=32, R=200, k=10, nq=16384, metric=api.METRIC_L2, rows=c3_rows, lo=0.0, hi=1e30),
    "emb": dict(d=768, nlist=4096, M=64, P=64, R=1000, k=10, nq=4096, metric=api.METRIC_IP, rows=emb_rows, lo=-1e30, hi=1e30),
}
DTYPES = ("float32", "float16", "sq8")
NRECALL = 1024


def build(S, base, ntrain, cc, pq, dtype):
    g = api.GammaHip(0)
    g.ivfpq_init(S["d"], S["nlist"], S["M"], 8, S["metric"], bucket_init_size=max(200, int(1.3 * len(base) / S["nlist"])))
    g.ivfpq_set_trained(cc, pq, None)
    g.raw_init(S["d"], dtype)
    if dtype == "sq8":
        g.raw_sq8_train(base[:ntrain])
    for c in range(0, len(base), 250000):
        g.raw_append(base[c:c + 250000])
        g.add(base[c:c + 250000], c)
    return g


def recall_at_k(I, truth):
    hit = sum(len(set(a[a >= 0].tolist()) & set(b.tolist())) for a, b in zip(I, truth))
    return hit / float(truth.size)


def measure(S, g, q, reps, calls, truth):
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
    first = I.cpu().numpy().copy()
    lat = []
    for i in range(300):
        t0 = time.perf_counter()
        g.ivfpq_search(q[i:i + 1], k, args)
        lat.append(1e6 * (time.perf_counter() - t0))
    st = g.raw_stats()
    return dict(qps_median=float(np.median(qps)), qps_min=min(qps), qps_max=max(qps),
                rerank_us_per_call_median=float(np.median(rr)), rerank_us_min=min(rr), rerank_us_max=max(rr),
                single_query_p50_us=float(np.median(lat[50:])), raw_elem_bytes=g.raw_elem_bytes(), raw_elem_type=g.raw_elem_type(),
                raw_store_bytes=st["capacity"] * S["d"] * g.raw_elem_bytes(), raw_rows_bytes=st["rows"] * S["d"] * g.raw_elem_bytes(),
                total_mem_bytes=g.total_mem_bytes(), recall_at_10=recall_at_k(first[:NRECALL], truth))


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
    q = S["rows"](2 * S["nq"], S["d"], 4321)
    ntrain = min(n, S["nlist"] * 40)
    cc, pq = api.train_ivfpq(base[:ntrain], S["nlist"], S["M"])
    res = dict(shape=a.shape, n=n, d=S["d"], nlist=S["nlist"], M=S["M"], nprobe=S["P"], recall_num=S["R"], k=S["k"],
               nq_call=S["nq"], calls=a.calls, reps=a.reps, recall_queries=NRECALL, sq8_range_rows=ntrain, build_s=None)
    truth = None
    for dtype in DTYPES:
        g = build(S, base, ntrain, cc, pq, dtype)
        try:
            if truth is None:   # flat search over the fp32 rows: the neighbours recall is counted against
                flat = api.SearchArgs(metric=S["metric"], min_score=S["lo"], max_score=S["hi"])
                truth = g.flat_search(q[:NRECALL], S["k"], flat)[1]
            res[dtype] = measure(S, g, q, a.reps, a.calls, truth)
        finally:
            g.close()
    res["build_s"] = round(time.time() - t0, 1)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
