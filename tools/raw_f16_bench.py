"""The float16 raw store against the fp32 one, same handle contents, one process ("Float16 raw store").

  python tools/raw_f16_bench.py --shape c3  [--n 1000000] [--out profiles/raw_f16_c3.json]
  python tools/raw_f16_bench.py --shape emb [--n 1000000]

c3 : n x 128 synth.sift_like, L2, nlist 4096, M 16, nprobe 32, recall_num 200, k 10, 16384-query device-pointer calls.  The data
     is lossless in fp16, so the results of the two stores must be identical: asserted.
emb: n x 768 synth.embedding_like, inner product, M 64, nprobe 64, recall_num 1000, k 10, 4096-query calls; recall@10 of both
     stores against the flat search over the fp32 rows on 1024 queries (reported).
Per store: queries/s (median of --reps repetitions, min - max), the re-rank stage's us per call (gamma_hip_profile_get, a pass
of its own), single-query p50, the store's bytes.  One JSON line."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from gamma_amd import api, synth

SHAPES = {
    "c3": dict(d=128, nlist=4096, M=16, P=32, R=200, k=10, nq=16384, metric=api.METRIC_L2, gen=synth.sift_like,
               lo=0.0, hi=1e30),
    "emb": dict(d=768, nlist=4096, M=64, P=64, R=1000, k=10, nq=4096, metric=api.METRIC_IP, gen=synth.embedding_like,
                lo=-1e30, hi=1e30),
}


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
               single_query_p50_us=float(np.median(lat[50:])), raw_elem_bytes=g.raw_elem_bytes(),
               raw_store_bytes=st["capacity"] * S["d"] * g.raw_elem_bytes(), raw_rows_bytes=st["rows"] * S["d"] * g.raw_elem_bytes(),
               total_mem_bytes=g.total_mem_bytes())
    return out, first, args


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
    base = S["gen"](n, d=S["d"], seed=1234)
    q = S["gen"](2 * S["nq"], d=S["d"], seed=4321)
    cc, pq = api.train_ivfpq(base[:min(n, S["nlist"] * 40)], S["nlist"], S["M"])
    res = dict(shape=a.shape, n=n, d=S["d"], nlist=S["nlist"], M=S["M"], nprobe=S["P"], recall_num=S["R"], k=S["k"],
               nq_call=S["nq"], calls=a.calls, reps=a.reps, build_s=None)
    firsts = {}
    for dtype in ("float32", "float16"):
        g = build(S, base, cc, pq, dtype)
        try:
            res[dtype], firsts[dtype], args = measure(S, g, q, a.reps, a.calls)
            if a.shape == "emb":
                NR = 1024
                if dtype == "float32":
                    _, If = g.flat_search(q[:NR], S["k"], api.SearchArgs(metric=S["metric"], min_score=S["lo"], max_score=S["hi"]))
                Ig = g.ivfpq_search(q[:NR], S["k"], args)[1]
                res[dtype]["recall_at_10"] = float(np.mean([len(set(Ig[i].tolist()) & set(If[i].tolist())) / float(S["k"])
                                                            for i in range(NR)]))
        finally:
            g.close()
    res["build_s"] = round(time.time() - t0, 1)
    same = firsts["float32"][0].tobytes() == firsts["float16"][0].tobytes() and np.array_equal(firsts["float32"][1], firsts["float16"][1])
    res["results_identical"] = bool(same)
    if a.shape == "c3":
        assert same, "c3 data is exact in fp16: the two stores must give identical results"
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
