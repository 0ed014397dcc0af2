"""4-bit IVFPQ workload P4: the data shape of C3 (1 M x 128, nlist 4096, nprobe 32, recall_num 200, re-rank, k = 10) with
M = 32 sub-quantizers at 4 bits (16-byte codes, like C3's), 16384-query device-pointer calls.  Beside it the same shape at 8
bits, M = 16, with the bounded scan off (GAMMA_HIP_NO_SCAN_BOUND=1 while that leg's handle is created: the plain scan on every
call; gamma_hip_set_scan_bound_feedback only stops the handle from backing off), as the point of comparison: the same code
bytes through the same plain path.
Prints one JSON line (and writes it to --out): queries/s, microseconds per stage (the handle's stage events), code bytes
per second of the scan, recall@10 against the flat search.
    python tools/pq4_bench.py [--n 1000000] [--steps 10] [--warmup 3] [--out profiles/pq4_p4_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run_leg(a, bits, M, base, q, flat_I):
    import torch

    from gamma_amd import api, synth  # noqa: F401
    if bits == 8:
        os.environ["GAMMA_HIP_NO_SCAN_BOUND"] = "1"   # read when the handle is created: the plain scan, as the 4-bit leg runs
    else:
        os.environ.pop("GAMMA_HIP_NO_SCAN_BOUND", None)
    g = api.GammaHip(0)
    d = base.shape[1]
    if bits == 4:
        g.ivfpq4_init(d, a.nlist, M, api.METRIC_L2, bucket_init_size=max(1000, a.n // a.nlist))
    else:
        g.ivfpq_init(d, a.nlist, M, 8, api.METRIC_L2, bucket_init_size=max(1000, a.n // a.nlist))
    t0 = time.time()
    cc, pq = g.ivfpq_train(base[:min(a.n, a.nlist * 64)], a.nlist, M)
    t_train = time.time() - t0
    g.ivfpq_set_trained(cc, pq, None)
    g.raw_init(d)
    g.raw_append(base)
    t0 = time.time()
    for i0 in range(0, a.n, 1 << 18):
        g.add(base[i0:i0 + (1 << 18)], i0)
    t_add = time.time() - t0
    k = 10
    args = api.SearchArgs(metric=api.METRIC_L2, nprobe=a.nprobe, recall_num=a.recall_num, has_rank=True,
                          min_score=-3e38, max_score=3e38)
    dx = torch.from_numpy(q).cuda()
    dD = torch.empty((a.nq, k), dtype=torch.float32, device="cuda")
    dI = torch.empty((a.nq, k), dtype=torch.int64, device="cuda")

    def dev():
        g.ivfpq_search_device(dx.data_ptr(), a.nq, k, args, dD.data_ptr(), dI.data_ptr())
    for _ in range(a.warmup):
        dev()
    g.synchronize()
    times = []
    for _ in range(a.steps):
        t0 = time.perf_counter()
        dev()
        g.synchronize()
        times.append(time.perf_counter() - t0)
    t_dev = float(np.median(times))
    I = dI.cpu().numpy()
    nf = flat_I.shape[0]
    recall = float(np.mean([len(set(I[i].tolist()) & set(flat_I[i].tolist())) / float(k) for i in range(nf)]))
    g.profile_enable(1)
    g.profile_reset()
    for _ in range(a.steps):
        dev()
    g.synchronize()
    prof = g.profile()
    g.profile_enable(0)
    stage_us = {name: round(v[0] / max(1, v[1]) * 1e3, 1) for name, v in prof.items()
                if isinstance(v, (tuple, list)) and len(v) >= 2 and v[1]}
    sizes = np.array([g.list_size(l) for l in range(a.nlist)], np.int64)
    # codes scanned: the probed lists' lengths over the call's coarse assignment
    st = g.last_stages(a.nq, a.nprobe, a.recall_num)
    ci = st["coarse_idx"]
    scanned = int(sizes[ci[ci >= 0]].sum())
    cs = g.code_size()
    scan_us = stage_us.get("scan", 0.0)
    out = {"bits": bits, "M": M, "code_size": cs, "train_s": round(t_train, 2), "add_s": round(t_add, 2),
           "device_qps": round(a.nq / t_dev), "device_ms_median": round(t_dev * 1e3, 3),
           "device_ms_min_max": [round(min(times) * 1e3, 3), round(max(times) * 1e3, 3)],
           "stage_us": stage_us, "codes_per_query": round(scanned / a.nq, 1),
           "scan_code_bytes_per_s": float("%.4g" % (scanned * cs / (scan_us * 1e-6))) if scan_us else None,
           "scan_gathers_per_s": float("%.4g" % (scanned * M / (scan_us * 1e-6))) if scan_us else None,
           "recall_at_10_vs_flat": round(recall, 4), "recall_queries": nf,
           "ties_not_honoured": g.ties_not_honoured()}
    g.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--nprobe", type=int, default=32)
    ap.add_argument("--recall_num", type=int, default=200)
    ap.add_argument("--nq", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--legs", default="4,8")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from gamma_amd import api, synth
    base = synth.sift_like(a.n, d=a.d, seed=1234)
    q = synth.sift_like(a.nq, d=a.d, seed=4321)
    # the exact neighbours of the first queries (flat search on the device)
    g = api.GammaHip(0)
    g.raw_init(a.d)
    g.raw_append(base)
    _, flat_I = g.flat_search(q[:1024], 10, api.SearchArgs(metric=api.METRIC_L2, min_score=-3e38, max_score=3e38))
    g.close()
    res = {"workload": "P4", "n": a.n, "d": a.d, "nlist": a.nlist, "nprobe": a.nprobe, "recall_num": a.recall_num,
           "nq": a.nq, "k": 10, "steps": a.steps}
    for leg in a.legs.split(","):
        bits = int(leg)
        res["pq%d" % bits] = run_leg(a, bits, 32 if bits == 4 else 16, base, q, flat_I)
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
