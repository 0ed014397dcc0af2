"""Binary IVF workload B1 (1 M synthetic clustered 256-bit codes, nlist 1024, nprobe 20), large batches: the list-major scan
(gamma_hip_binivf_set_lm_scan on, min_nq 1, scan mode 0) against the switch off under the default scan mode -- the kernels
a handle runs without it: the spread chain up to its auto_max_nq queries, one wave per query beyond -- on ONE handle in one
process, device-pointer calls.  Per shape (nq in 1024 .. 65536, k = 10 and 100): the two answers are asserted byte-identical;
the time per call is the median of `reps` repetitions (each a window of calls that ends in a device synchronise, off and on
alternating), with min - max; the per-stage split (coarse | inverse index + table + histograms + bounds | collect | replay)
comes from the handle's stage events in a separate profiled run, with the units, chunks and candidates per query.  Prints
one JSON line; "faster" at a shape means the new path's slowest repetition beats the baseline's fastest.
    python tools/binivf_lm_bench.py [--n 1000000] [--reps 5] [--out profiles/binivf_lm_b1.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.binivf_bench import clustered  # noqa: E402

NQS = (1024, 4096, 16384, 65536)
KS = (10, 100)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--nbits", type=int, default=256)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nqs", default=",".join(str(v) for v in NQS))
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    nqs = tuple(int(v) for v in a.nqs.split(","))
    import torch

    from gamma_amd import api
    chunk_rows, qtile, auto_min_nq = api.binivf_lm_shape()
    base = clustered(a.n, a.nbits, 4096, 0.06, 1)
    q = clustered(max(nqs), a.nbits, 4096, 0.06, 2)
    g = api.GammaHip(0)
    cc = g.binivf_train(base[:a.nlist * 256], a.nlist)
    g.binivf_init(a.nbits, a.nlist, bucket_init_size=max(1000, a.n // a.nlist))
    g.binivf_set_trained(cc)
    g.binivf_add(base, 0)
    dx = torch.from_numpy(q).cuda()
    args = api.SearchArgs(nprobe=a.nprobe)
    res = {"workload": "B1", "n": a.n, "nbits": a.nbits, "nlist": a.nlist, "nprobe": a.nprobe, "reps": a.reps,
           "chunk_rows": chunk_rows, "query_tile": qtile, "auto_min_nq_built": auto_min_nq,
           "longest_list": g.max_list_len(), "shapes": []}

    def switch(on):
        g.binivf_set_scan_mode(0 if on else -1)
        g.binivf_set_lm_scan(on, min_nq=1)

    faster = {}
    for k in KS:
        for nq in nqs:
            dD = [torch.empty((nq, k), dtype=torch.float32, device="cuda") for _ in range(2)]
            dI = [torch.empty((nq, k), dtype=torch.int64, device="cuda") for _ in range(2)]

            def call(on):
                g.binivf_search_device(dx.data_ptr(), nq, k, args, dD[on].data_ptr(), dI[on].data_ptr())

            for on in (0, 1):   # warm-up of the shape (workspaces grow here), and the answers
                switch(on)
                for _ in range(2):
                    call(on)
            torch.cuda.synchronize()
            same = bool(torch.equal(dI[0], dI[1]) and torch.equal(dD[0].view(torch.int32), dD[1].view(torch.int32)))
            assert same, "the list-major answer differs at nq %d k %d" % (nq, k)
            iters = int(max(3, min(300, 16384 // nq)))
            t = {0: [], 1: []}
            for _ in range(a.reps):
                for on in (0, 1):
                    switch(on)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(iters):
                        call(on)
                    torch.cuda.synchronize()
                    t[on].append((time.perf_counter() - t0) / iters * 1e6)
            row = {"nq": nq, "k": k, "iters": iters, "identical": same}
            for on in (0, 1):   # stage events and counters: a separate run, they cost a little
                switch(on)
                g.profile_enable(1)
                g.profile_reset()
                g.binivf_stats(reset=True)
                g.binivf_lm_stats(reset=True)
                for _ in range(iters):
                    call(on)
                torch.cuda.synchronize()
                prof = g.profile()
                nqd, adm = g.binivf_stats(reset=True)
                lq, lu, lch, lcand, lfall = g.binivf_lm_stats(reset=True)
                g.profile_enable(0)
                us = {s: round(prof[s][0] / max(1, prof[s][1]) * 1e3, 1) for s in ("coarse", "tables", "scan", "select")}
                v = np.array(t[on])
                row["on" if on else "off"] = {
                    "us_median": round(float(np.median(v)), 1), "us_min": round(float(v.min()), 1),
                    "us_max": round(float(v.max()), 1), "stage_us": us,
                    "admissions_per_query": round(adm / max(1, nqd), 2), "lm_queries": lq,
                    "units_per_call": lu // iters, "chunks_per_query": round(lch / max(1, lq), 1),
                    "candidates_per_query": round(lcand / max(1, lq), 1), "fell_back": lfall}
            row["on_faster_outside_spreads"] = bool(max(t[1]) < min(t[0]))
            faster[(nq, k)] = row["on_faster_outside_spreads"]
            res["shapes"].append(row)
            print("nq %5d k %3d  off %9.1f us (%.1f - %.1f)  on %9.1f us (%.1f - %.1f)  %s  stages on %s" % (
                nq, k, row["off"]["us_median"], row["off"]["us_min"], row["off"]["us_max"],
                row["on"]["us_median"], row["on"]["us_min"], row["on"]["us_max"],
                "faster" if faster[(nq, k)] else "not faster", row["on"]["stage_us"]), file=sys.stderr, flush=True)
    # the smallest measured nq from which the new path is faster at both k, at that size and at every larger one
    from_nq = 0
    for nq in sorted(nqs, reverse=True):
        if not all(faster[(nq, k)] for k in KS):
            break
        from_nq = nq
    res["auto_min_nq_measured"] = from_nq
    g.close()
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
