"""Exact Hamming search on workload B1's data (1 M synthetic clustered 256-bit codes): the binary flat store
(gamma_hip_binflat_search) against the exact route there was before it -- a binary IVF handle with nlist 1, every code in
its single list, nprobe 1 (k_bin_scan: one wave per query over all rows).  Both are built in this process, their results are
asserted byte-identical at every shape, and one JSON line per shape is printed: ms per device-pointer call as the median of
`reps` repetitions of `calls` calls with min - max (the two routes alternate), the flat search's counters per query and its
stage times (hist + bounds / collect / replay, from the handle's stage events in a run of their own), and the bytes the
design reads: hist reads every code once per query TILE, collect at most once more.
    python tools/binflat_bench.py [--n 1000000] [--nq 1,64,1024,16384] [--k 10,100] [--reps 5] [--calls 4]
Shapes above --baseline-full-nq time the baseline with one call per repetition (it walks nq x n rows one wave per query)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.binivf_bench import clustered  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--nbits", type=int, default=256)
    ap.add_argument("--nq", default="1,64,1024,16384")
    ap.add_argument("--k", default="10,100")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--baseline-full-nq", type=int, default=1024)
    a = ap.parse_args()
    import torch

    from gamma_amd import api
    nqs = [int(v) for v in a.nq.split(",")]
    ks = [int(v) for v in a.k.split(",")]
    cs = a.nbits // 8
    base = clustered(a.n, a.nbits, 4096, 0.06, 1)
    q = clustered(max(nqs), a.nbits, 4096, 0.06, 2)
    flat = api.GammaHip(0)
    flat.binflat_init(a.nbits)
    flat.binflat_append(base)
    ivf = api.GammaHip(0)   # the exact route before the flat store: one list that holds every code in vid order
    ivf.binivf_init(a.nbits, 1, bucket_init_size=a.n)
    ivf.binivf_set_trained(base[:1])
    ivf.binivf_add(base, 0)
    chunk = flat.binflat_chunk_rows()
    dx = torch.from_numpy(q).cuda()
    args = api.SearchArgs(nprobe=1)

    def timed(fn, calls):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / calls * 1e3

    for nq in nqs:
        for k in ks:
            dD = [torch.empty((nq, k), dtype=torch.float32, device="cuda") for _ in range(2)]
            dI = [torch.empty((nq, k), dtype=torch.int64, device="cuda") for _ in range(2)]

            def run_flat():
                flat.binflat_search_device(dx.data_ptr(), nq, k, args, dD[0].data_ptr(), dI[0].data_ptr())

            def run_base():
                ivf.binivf_search_device(dx.data_ptr(), nq, k, args, dD[1].data_ptr(), dI[1].data_ptr())
            run_flat()   # warm-up of both routes at this shape, and the comparison
            run_base()
            torch.cuda.synchronize()
            assert torch.equal(dI[0], dI[1]), "labels differ at nq %d k %d" % (nq, k)
            assert dD[0].cpu().numpy().tobytes() == dD[1].cpu().numpy().tobytes(), "distances differ at nq %d k %d" % (nq, k)
            bcalls = a.calls if nq <= a.baseline_full_nq else 1
            tf, tb = [], []
            for _ in range(a.reps):
                tf.append(timed(run_flat, a.calls))
                tb.append(timed(run_base, bcalls))
            flat.profile_enable(1)
            flat.profile_reset()
            flat.binflat_stats(reset=True)
            for _ in range(a.calls):
                run_flat()
            torch.cuda.synchronize()
            prof = flat.profile()
            queries, cand, adm, sub = flat.binflat_stats(reset=True)
            flat.profile_enable(0)
            tile = 1 if nq <= 1 else (4 if nq <= 4 else 8)
            tiles = (nq + tile - 1) // tile
            print(json.dumps({
                "workload": "B1-flat", "n": a.n, "nbits": a.nbits, "nq": nq, "k": k, "identical": True,
                "flat_ms": round(float(np.median(tf)), 4), "flat_ms_min": round(min(tf), 4), "flat_ms_max": round(max(tf), 4),
                "baseline_ms": round(float(np.median(tb)), 4), "baseline_ms_min": round(min(tb), 4),
                "baseline_ms_max": round(max(tb), 4), "baseline_calls_per_rep": bcalls,
                "speedup": round(float(np.median(tb)) / float(np.median(tf)), 2),
                "outside_spreads": bool(max(tf) < min(tb)),
                "candidates_per_query": round(cand / max(1, queries), 1),
                "admissions_per_query": round(adm / max(1, queries), 2),
                "sub_batches_per_call": round(sub / a.calls, 2), "chunk_rows": chunk,
                "hist_bounds_ms": round(prof["coarse"][0] / a.calls, 4), "collect_ms": round(prof["scan"][0] / a.calls, 4),
                "replay_ms": round(prof["select"][0] / a.calls, 4),
                "code_bytes_read_flat": 2 * tiles * a.n * cs, "code_bytes_read_baseline": nq * a.n * (cs + 8),
            }), flush=True)
    flat.close()
    ivf.close()


if __name__ == "__main__":
    main()
