"""Binary IVF workload B1 (1 M synthetic clustered 256-bit codes, nlist 1024, nprobe 20): the scan of one wave per query
(scan mode 0) against the scan spread over the device (scan mode 1), on ONE handle in one process, device-pointer calls.
Per shape (nq in 1 .. 4096, k = 10 and 100): the two answers are asserted byte-identical; the time per call is the median of
`reps` repetitions (each a window of calls that ends in a device synchronise, the two modes alternating), with min - max;
the per-stage split comes from the handle's stage events in a separate profiled run (mode 0: coarse step | k_bin_scan; mode
1: coarse step | chunk table + histograms + bounds | collect | replay), together with the chain's chunks and candidates per
query.  Prints one JSON line; the verdicts compare the spreads, not the medians: mode 1 is "faster" at a shape only where its
slowest repetition beats mode 0's fastest.
    python tools/binivf_spread_bench.py [--n 1000000] [--reps 5] [--out profiles/binivf_spread_b1.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.binivf_bench import clustered  # noqa: E402

NQS = (1, 8, 64, 256, 1024, 4096)
KS = (10, 100)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--nbits", type=int, default=256)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch

    from gamma_amd import api
    chunk_rows, auto_max_nq = api.binivf_scan_shape()
    base = clustered(a.n, a.nbits, 4096, 0.06, 1)
    q = clustered(max(NQS), a.nbits, 4096, 0.06, 2)
    g = api.GammaHip(0)
    cc = g.binivf_train(base[:a.nlist * 256], a.nlist)
    g.binivf_init(a.nbits, a.nlist, bucket_init_size=max(1000, a.n // a.nlist))
    g.binivf_set_trained(cc)
    g.binivf_add(base, 0)
    sizes = np.array([g.list_size(l) for l in range(a.nlist)], np.int64)
    dx = torch.from_numpy(q).cuda()
    args = api.SearchArgs(nprobe=a.nprobe)
    res = {"workload": "B1", "n": a.n, "nbits": a.nbits, "nlist": a.nlist, "nprobe": a.nprobe, "reps": a.reps,
           "chunk_rows": chunk_rows, "auto_max_nq_built": auto_max_nq, "longest_list": int(sizes.max()),
           "mean_list": round(float(sizes.mean()), 1), "shapes": []}
    faster = {}
    for k in KS:
        for nq in NQS:
            dD = [torch.empty((nq, k), dtype=torch.float32, device="cuda") for _ in range(2)]
            dI = [torch.empty((nq, k), dtype=torch.int64, device="cuda") for _ in range(2)]

            def call(mode):
                g.binivf_search_device(dx.data_ptr(), nq, k, args, dD[mode].data_ptr(), dI[mode].data_ptr())

            for mode in (0, 1):   # warm-up of the shape (workspaces grow here), and the answers
                g.binivf_set_scan_mode(mode)
                for _ in range(3):
                    call(mode)
            torch.cuda.synchronize()
            same = bool(torch.equal(dI[0], dI[1]) and torch.equal(dD[0].view(torch.int32), dD[1].view(torch.int32)))
            assert same, "mode 1 differs from mode 0 at nq %d k %d" % (nq, k)
            iters = int(max(5, min(300, 16384 // nq)))
            t = {0: [], 1: []}
            for _ in range(a.reps):
                for mode in (0, 1):
                    g.binivf_set_scan_mode(mode)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(iters):
                        call(mode)
                    torch.cuda.synchronize()
                    t[mode].append((time.perf_counter() - t0) / iters * 1e6)
            row = {"nq": nq, "k": k, "iters": iters, "identical": same}
            for mode in (0, 1):   # stage events and counters: a separate run, they cost a little
                g.binivf_set_scan_mode(mode)
                g.profile_enable(1)
                g.profile_reset()
                g.binivf_stats(reset=True)
                g.binivf_scan_stats(reset=True)
                for _ in range(iters):
                    call(mode)
                torch.cuda.synchronize()
                prof = g.profile()
                nqs, adm = g.binivf_stats(reset=True)
                sq, sch, scand, sfall = g.binivf_scan_stats(reset=True)
                g.profile_enable(0)
                us = {s: round(prof[s][0] / max(1, prof[s][1]) * 1e3, 1) for s in ("coarse", "tables", "scan", "select")}
                v = np.array(t[mode])
                row["mode%d" % mode] = {
                    "us_median": round(float(np.median(v)), 1), "us_min": round(float(v.min()), 1),
                    "us_max": round(float(v.max()), 1), "stage_us": us,
                    "admissions_per_query": round(adm / max(1, nqs), 2),
                    "spread_queries": sq, "chunks_per_query": round(sch / max(1, sq), 1),
                    "candidates_per_query": round(scand / max(1, sq), 1), "fell_back": sfall}
            row["mode1_faster_outside_spreads"] = bool(max(t[1]) < min(t[0]))
            faster[(nq, k)] = row["mode1_faster_outside_spreads"]
            res["shapes"].append(row)
            print("nq %5d k %3d  mode 0 %9.1f us (%.1f - %.1f)  mode 1 %9.1f us (%.1f - %.1f)  %s" % (
                nq, k, row["mode0"]["us_median"], row["mode0"]["us_min"], row["mode0"]["us_max"],
                row["mode1"]["us_median"], row["mode1"]["us_min"], row["mode1"]["us_max"],
                "faster" if row["mode1_faster_outside_spreads"] else "not faster"), file=sys.stderr, flush=True)
    both = [nq for nq in NQS if all(faster[(nq, k)] for k in KS)]
    res["auto_max_nq_measured"] = max(both) if both else 0
    res["target_nq1"] = "HIT" if all(faster[(1, k)] for k in KS) else "MISS"
    res["target_nq64"] = "HIT" if all(faster[(64, k)] for k in KS) else "MISS"
    g.close()
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
