"""Binary IVF workload B1: 1 M synthetic clustered 256-bit codes, nlist 1024, nprobe 20, k = 10 and 100.  Modes: 16384-query
device-pointer calls, host-buffer calls, single-query latency.  Prints one JSON line: q/s, microseconds per stage (coarse
step, scan; from the handle's stage events), codes scanned per second, mean heap admissions per query (the serial part),
and the scan time against two floors -- the popcount work and the code + id bytes read at HBM's 8 TB/s (the lists may
sit in L2 / MALL instead, so neither floor is the scan's actual bound).
    python tools/binivf_bench.py [--n 1000000] [--steps 10] [--warmup 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def clustered(n, nbits, ncenters, flip, seed):
    rng = np.random.default_rng(seed)
    cs = nbits // 8
    centers = rng.integers(0, 256, size=(ncenters, cs), dtype=np.uint8)
    out = np.empty((n, cs), np.uint8)
    for i0 in range(0, n, 1 << 17):
        m = min(1 << 17, n - i0)
        bits = np.unpackbits(centers[rng.integers(0, ncenters, m)], axis=1, bitorder="little")
        bits ^= (rng.random(bits.shape) < flip).astype(np.uint8)
        out[i0:i0 + m] = np.packbits(bits, axis=1, bitorder="little")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--nbits", type=int, default=256)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, default=20)
    ap.add_argument("--nq", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch

    from gamma_amd import api
    base = clustered(a.n, a.nbits, 4096, 0.06, 1)
    q = clustered(a.nq, a.nbits, 4096, 0.06, 2)
    g = api.GammaHip(0)
    t0 = time.time()
    cc = g.binivf_train(base[:a.nlist * 256], a.nlist)
    t_train = time.time() - t0
    g.binivf_init(a.nbits, a.nlist, bucket_init_size=max(1000, a.n // a.nlist))
    g.binivf_set_trained(cc)
    t0 = time.time()
    g.binivf_add(base, 0)
    t_add = time.time() - t0
    cs = a.nbits // 8
    dx = torch.from_numpy(q).cuda()
    res = {"workload": "B1", "n": a.n, "nbits": a.nbits, "nlist": a.nlist, "nprobe": a.nprobe, "nq": a.nq,
           "train_s": round(t_train, 3), "add_s": round(t_add, 3)}
    sizes = np.array([g.list_size(l) for l in range(a.nlist)], np.int64)
    for k in (10, 100):
        args = api.SearchArgs(nprobe=a.nprobe)
        dD = torch.empty((a.nq, k), dtype=torch.float32, device="cuda")
        dI = torch.empty((a.nq, k), dtype=torch.int64, device="cuda")

        def dev():
            g.binivf_search_device(dx.data_ptr(), a.nq, k, args, dD.data_ptr(), dI.data_ptr())
        for _ in range(a.warmup):
            dev()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            dev()
        torch.cuda.synchronize()
        t_dev = (time.perf_counter() - t0) / a.steps
        # per-stage times and heap admissions (stage events and counters: a separate run, they cost a little)
        g.profile_enable(1)
        g.profile_reset()
        g.binivf_stats(reset=True)
        for _ in range(a.steps):
            dev()
        torch.cuda.synchronize()
        prof = g.profile()
        nqs, adm = g.binivf_stats(reset=True)
        g.profile_enable(0)
        coarse_ms = prof["coarse"][0] / max(1, prof["coarse"][1])
        scan_ms = prof["scan"][0] / max(1, prof["scan"][1])
        # codes scanned: the probed lists' lengths (from the coarse assignment of the queries)
        _, probes = g.binivf_assign(q, a.nprobe)
        scanned = int(sizes[probes[probes >= 0]].sum())
        for _ in range(a.warmup):
            g.binivf_search(q, k, args)
        t0 = time.perf_counter()
        for _ in range(max(1, a.steps // 2)):
            g.binivf_search(q, k, args)
        t_host = (time.perf_counter() - t0) / max(1, a.steps // 2)
        lat = []
        for i in range(200 + a.warmup):
            t0 = time.perf_counter()
            g.binivf_search(q[i:i + 1], k, args)
            lat.append(time.perf_counter() - t0)
        lat = np.array(lat[a.warmup:]) * 1e6
        bytes_alg = scanned * (cs + 8)
        floor_bw_us = bytes_alg / 8e12 * 1e6
        # popcount floor: an XOR and a v_bcnt per 32-bit word of every code; a CU issues 128 lane-ops per clock (4 SIMDs,
        # a wave64 VALU instruction over 2 cycles), 256 CUs at 2.4 GHz
        floor_pop_us = scanned * (cs // 4) * 2 / (256 * 128 * 2.4e9) * 1e6
        res["k%d" % k] = {
            "device_qps": round(a.nq / t_dev), "device_ms": round(t_dev * 1e3, 3),
            "host_qps": round(a.nq / t_host), "host_ms": round(t_host * 1e3, 3),
            "single_query_us_p50": round(float(np.percentile(lat, 50)), 1),
            "single_query_us_p99": round(float(np.percentile(lat, 99)), 1),
            "coarse_us": round(coarse_ms * 1e3, 1), "scan_us": round(scan_ms * 1e3, 1),
            "codes_scanned_per_s": float("%.4g" % (scanned / t_dev)),
            "codes_per_query": round(scanned / a.nq, 1),
            "heap_admissions_per_query": round(adm / max(1, nqs), 2),
            "scan_floor_hbm_bytes_us": round(floor_bw_us, 1), "scan_floor_popcount_us": round(floor_pop_us, 1),
            "larger_floor": "hbm_bytes" if floor_bw_us >= floor_pop_us else "popcount",
        }
    g.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
