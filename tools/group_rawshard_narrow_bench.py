#!/usr/bin/env python3
"""Raw rows sharded with their lists, fp32 beside narrow rows: the in-process group of --members
handles, every one on device 0, over C3's data shape (SIFT-like, d = 128) at --n vectors -- lists sharded by owner, every raw
row once at the owner of its list ("raw_placement": "sharded"), re-rank on, calls of --nq queries through device pointers.
--raw-dtype float32 runs on any build that has the sharded raw placement; uint8 / float16 need gamma_hip_set_sparse_narrow_rows.
Prints one JSON line: the step time (every run of --runs, and their median), the members' row bytes (gamma_hip_raw_stats:
rows held and rows reserved, times d x element size) and recall@10 against the exact neighbours of the fp32 vectors.
Members sharing one GPU run one after another where members on GPUs of their own would run side by side, and their exchanges
are device-to-device copies: the numbers compare the row types with each other and say nothing about xGMI."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--raw-dtype", default="float32", choices=["float32", "float16", "uint8"])
    ap.add_argument("--members", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--nq", type=int, default=4096, help="queries per call (the whole group)")
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--m", type=int, default=16)
    ap.add_argument("--nprobe", type=int, default=32)
    ap.add_argument("--recall-num", type=int, default=200)
    ap.add_argument("--k", type=int, default=10)
    a = ap.parse_args()
    import torch
    from gamma_amd import api, synth
    W, d = a.members, 128
    esz = {"float32": 4, "float16": 2, "uint8": 1}[a.raw_dtype]
    base = synth.sift_like(a.n, d=d, seed=1234)                   # integers in [0, 255]: uint8 and float16 hold them exactly
    nb = 4
    queries = synth.sift_like(a.nq * nb, d=d, seed=4321)
    cc, pq = api.train_ivfpq(base[:min(a.n, a.nlist * 64)], a.nlist, a.m)
    grp = api.GammaHipGroup([0] * W)
    grp.set_placement(False)
    for m in grp.members:
        m.ivfpq_init(d, a.nlist, a.m, 8, api.METRIC_L2, bucket_init_size=max(1000, int(2.5 * a.n / a.nlist / W)))
        m.ivfpq_set_trained(cc, pq, None)
        if a.raw_dtype == "float32":
            m.raw_init(d)
        else:
            m.raw_init(d, a.raw_dtype)
            m.set_sparse_narrow_rows(True)
    grp.set_raw_placement(True)
    lno, _ = grp.members[0].encode(base[:min(a.n, 262144)])
    grp.set_owners(np.bincount(lno, minlength=a.nlist))
    t0 = time.time()
    for i0 in range(0, a.n, 100000):
        grp.add(base[i0:i0 + 100000], i0)
    build_s = time.time() - t0
    args = api.SearchArgs(metric=api.METRIC_L2, nprobe=a.nprobe, recall_num=a.recall_num, has_rank=True, min_score=0.0,
                          max_score=1e30)
    dev0 = torch.device("cuda", 0)
    d_q = torch.from_numpy(queries).to(dev0)
    d_D = torch.empty((a.nq, a.k), dtype=torch.float32, device=dev0)
    d_I = torch.empty((a.nq, a.k), dtype=torch.int64, device=dev0)
    torch.cuda.synchronize()

    def step(i):
        xb = d_q[(i % nb) * a.nq:(i % nb + 1) * a.nq]
        grp.ivfpq_search_device(xb.data_ptr(), a.nq, a.k, args, d_D.data_ptr(), d_I.data_ptr())

    for i in range(a.warmup):
        step(i)
    torch.cuda.synchronize()
    runs = []
    for _ in range(a.runs):
        t0 = time.perf_counter()
        for i in range(a.steps):
            step(a.warmup + i)
        torch.cuda.synchronize()
        runs.append((time.perf_counter() - t0) / a.steps * 1e3)
    nrq = 500
    xb = queries[((a.warmup + a.steps - 1) % nb) * a.nq:][:nrq]
    tb = torch.from_numpy(base).to(dev0)
    If = torch.topk((tb * tb).sum(1)[None, :] - 2.0 * (torch.from_numpy(xb).to(dev0) @ tb.T), a.k, largest=False).indices.cpu().numpy()
    del tb
    Ig = d_I[:nrq].cpu().numpy()
    recall = sum(len(set(Ig[i].tolist()) & set(If[i].tolist())) for i in range(nrq)) / float(nrq * a.k)
    stats = [m.raw_stats() for m in grp.members]
    ms = statistics.median(runs)
    out = {"metric": "ms per call of %d queries, sharded group of %d members on one GPU, raw rows %s" % (a.nq, W, a.raw_dtype),
           "value": round(ms, 4), "unit": "ms", "higher_is_better": False, "ms_per_step_runs": [round(r, 4) for r in runs],
           "queries_per_s": round(a.nq / ms * 1e3, 1), "steps": a.steps, "warmup": a.warmup, "raw_dtype": a.raw_dtype,
           "row_bytes_held": [s["rows"] * d * esz for s in stats], "row_bytes_reserved": [s["capacity"] * d * esz for s in stats],
           "row_bytes_held_total": sum(s["rows"] for s in stats) * d * esz, "rows_in_place": [s["in_place"] for s in stats],
           "device_bytes": grp.total_mem_bytes(), "recall_at_10": round(recall, 4), "build_s": round(build_s, 1),
           "config": {"n": a.n, "d": d, "nlist": a.nlist, "M": a.m, "nprobe": a.nprobe, "recall_num": a.recall_num, "k": a.k,
                      "note": "every member on device 0: nothing here speaks about xGMI"}}
    print(json.dumps(out), flush=True)
    grp.close()


if __name__ == "__main__":
    main()
