#!/usr/bin/env python3
"""IVFFLAT over the in-process group with rows sharded with their lists, the members holding their rows as fp32, float16 or uint8
(DESIGN section 33), at README's IVFFLAT shape: 1 M x 128 integer-valued rows (exact in all three types, so every configuration
holds the same numbers), nlist 4096, nprobe 32, k 10, batches of 16384 queries through gamma_hip_group_ivfflat_search_device.

EVERY MEMBER SHARES THE ONE GPU.  The members' kernels queue on the same device and the "exchange" is a copy inside one memory:
the figures compare the row types on the same silicon -- they say nothing about scaling over xGMI.

The three groups live in one process and are timed alternately: `rounds` rounds of `calls` calls each per row type, a host clock
around calls that end synchronised; per type the median of the rounds' means, the rounds themselves, the bytes of rows the members
hold and the group's device bytes.  The narrow groups' results are compared with the fp32 group's, byte for byte.
usage on the GPU box: python tools/ivfflat_group_rows_bench.py [members] [nq] [rounds] [calls]"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gamma_amd import api, synth  # noqa: E402

N, D, NLIST, P, K = 1000000, 128, 4096, 32, 10
DTYPES = ["float32", "float16", "uint8"]
ESZ = {"float32": 4, "float16": 2, "uint8": 1}


def make_group(W, dtype, cc, base, bucket):
    grp = api.GammaHipGroup([0] * W)
    for m in grp.members:
        m.ivfflat_init(D, NLIST, api.METRIC_L2, bucket_init_size=bucket)
        m.ivfflat_set_trained(cc)
        m.raw_init(D, dtype)
        if dtype != "float32":
            m.set_ivfflat_narrow_rows(True)
            m.set_sparse_narrow_rows(True)
    grp.set_raw_placement(True)
    grp.set_owners(None)
    for i0 in range(0, len(base), 1 << 16):
        grp.add(base[i0:i0 + (1 << 16)], i0)
    return grp


def main():
    W = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    nq = int(sys.argv[2]) if len(sys.argv) > 2 else 16384
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    calls = int(sys.argv[4]) if len(sys.argv) > 4 else 20
    if not torch.cuda.is_available():
        raise SystemExit("ivfflat_group_rows_bench: no GPU -- nothing is measured without one")
    dev = torch.device("cuda", 0)
    base = synth.sift_like(N, d=D, seed=1234)
    q = synth.sift_like(nq, d=D, seed=4321)
    cc, _ = api.train_ivfpq(base[:NLIST * 64], NLIST, 16)
    args = api.SearchArgs(metric=api.METRIC_L2, nprobe=P, min_score=0.0, max_score=1e30)
    dq = torch.from_numpy(q).to(dev)
    out = {t: (torch.empty((nq, K), dtype=torch.float32, device=dev), torch.empty((nq, K), dtype=torch.int64, device=dev))
           for t in DTYPES}
    bucket = max(1000, int(2.5 * N / NLIST))
    groups = {t: make_group(W, t, cc, base, bucket) for t in DTYPES}

    def run(t):
        groups[t].ivfflat_search_device(dq.data_ptr(), nq, K, args, out[t][0].data_ptr(), out[t][1].data_ptr())   # synchronous

    for t in DTYPES:      # warm: every workspace sized, every code object loaded
        run(t)
        run(t)
    torch.cuda.synchronize()
    ms = {t: [] for t in DTYPES}
    for _ in range(rounds):
        for t in DTYPES:
            t0 = time.time()
            for _ in range(calls):
                run(t)
            ms[t].append((time.time() - t0) / calls * 1e3)
    ref = (out["float32"][0].cpu().numpy(), out["float32"][1].cpu().numpy())
    for t in DTYPES:
        g = groups[t]
        live = [m.raw_sparse_stats()["live"] for m in g.members]
        Dt, It = out[t][0].cpu().numpy(), out[t][1].cpu().numpy()
        print(json.dumps({"rows": t, "members": W, "nq": nq, "rounds": rounds, "calls_per_round": calls,
                          "ms_per_call_median": round(float(np.median(ms[t])), 3), "ms_per_call_rounds": [round(v, 3) for v in ms[t]],
                          "vs_float32": round(float(np.median(ms[t]) / np.median(ms["float32"])), 3),
                          "row_bytes_per_member": [int(n) * D * ESZ[t] for n in live], "row_bytes": int(sum(live)) * D * ESZ[t],
                          "group_device_bytes": int(g.total_mem_bytes()),
                          "equals_float32_group": bool(Dt.tobytes() == ref[0].tobytes() and It.tobytes() == ref[1].tobytes()),
                          "note": "members share one GPU: no statement about scaling over xGMI"}), flush=True)
    for g in groups.values():
        g.close()


if __name__ == "__main__":
    main()
