#!/usr/bin/env python3
"""IVFFLAT over the in-process group at README's IVFFLAT shape (1 M x 128, nlist 4096, nprobe 32, k 10, batches of 16384
queries): one handle against groups of 2 and 4 members, rows replicated and rows sharded with their lists.

EVERY MEMBER SHARES THE ONE GPU.  The members' kernels queue on the same device and the "exchange" is a copy inside one memory:
the figures say what the sharded path costs beside one handle on the same silicon and where its time goes -- they say nothing
about scaling over xGMI, and no speed-up is expected of the emulation.

Per configuration: wall time per gamma_hip_group_ivfflat_search_device call, and the share of the phases measured on the
building blocks (gamma_hip_ivfflat_search_shard / _merge / _shard_export / _merge_replay on the group's own members, driven in
the group's order with a device synchronisation after each phase): scan (coarse + shard search of every member), exchange (the
[W][nq][k] tables and cut flags gathered), merge, tie phase (export + replay of the flagged queries).
usage on the GPU box: python tools/ivfflat_group_bench.py [nq] [calls]"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gamma_amd import api, synth  # noqa: E402

N, D, NLIST, P, K = 1000000, 128, 4096, 32, 10


def fill(target, base, members=None, sharded=False):
    for i0 in range(0, N, 1 << 16):
        xb = base[i0:i0 + (1 << 16)]
        if members is None:
            target.raw_append(xb)
        elif not sharded:
            for m in members:
                m.raw_append(xb)
        target.add(xb, i0)


def timed(fn, calls):
    fn()
    fn()
    t0 = time.time()
    for _ in range(calls):
        fn()
    return (time.time() - t0) / calls


def phases(members, dq, nq, args):
    """the group's sequence on its own members, one phase at a time (seconds per phase, flagged queries)"""
    W = len(members)
    dev = dq.device
    d = dq.shape[1]
    cd = torch.zeros((nq, P), dtype=torch.float32, device=dev)
    pr = torch.zeros((nq, P), dtype=torch.int32, device=dev)
    rd = [torch.zeros((nq, K), dtype=torch.float32, device=dev) for _ in members]
    ri = [torch.zeros((nq, K), dtype=torch.int64, device=dev) for _ in members]
    cf = [torch.zeros((nq,), dtype=torch.uint8, device=dev) for _ in members]
    Dm = torch.zeros((nq, K), dtype=torch.float32, device=dev)
    Im = torch.zeros((nq, K), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    t = {}
    t0 = time.time()
    members[0].ivfflat_coarse_device(dq.data_ptr(), nq, args, cd.data_ptr(), pr.data_ptr())
    members[0].synchronize()
    for m, a, b, c in zip(members, rd, ri, cf):
        m.ivfflat_search_shard(dq.data_ptr(), nq, cd.data_ptr(), pr.data_ptr(), K, args, a.data_ptr(), b.data_ptr())
        m.ivfpq_shard_cut_flags(nq, c.data_ptr())
    for m in members:
        m.synchronize()
    t["scan"] = time.time() - t0
    t0 = time.time()
    all_d, all_i, all_c = torch.stack(rd).contiguous(), torch.stack(ri).contiguous(), torch.stack(cf).contiguous()
    torch.cuda.synchronize()
    t["exchange"] = time.time() - t0
    t0 = time.time()
    own = members[0]
    own.ivfpq_merge_set_shard_flags(all_c.data_ptr())
    own.ivfflat_merge(W, nq, K, args, all_d.data_ptr(), all_i.data_ptr(), 0, nq, Dm.data_ptr(), Im.data_ptr())
    nf, d_list = own.ivfpq_merge_flagged()
    own.synchronize()
    t["merge"] = time.time() - t0
    t0 = time.time()
    for f0 in range(0, nf, 256):
        n = min(256, nf - f0)
        xf = torch.empty((n, d), dtype=torch.float32, device=dev)
        pf = torch.empty((n, P), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        own.gather_rows(dq.data_ptr(), d, d_list + 4 * f0, n, xf.data_ptr())
        own.gather_rows(pr.data_ptr(), P, d_list + 4 * f0, n, pf.data_ptr())
        own.synchronize()
        stride = max(4, (max(m.ivfflat_shard_export_rows(n, pf.data_ptr(), args) for m in members) + 3) // 4 * 4)
        vals = torch.empty((W, n, stride), dtype=torch.float32, device=dev)
        ids = torch.empty((W, n, stride), dtype=torch.int64, device=dev)
        off = torch.empty((W, n, P + 1), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        for s, m in enumerate(members):
            m.ivfflat_shard_export(n, xf.data_ptr(), pf.data_ptr(), stride, args, vals[s].data_ptr(), ids[s].data_ptr(),
                                   off[s].data_ptr())
            m.synchronize()
        own.ivfflat_merge_replay(W, n, dq.data_ptr(), stride, vals.data_ptr(), ids.data_ptr(), off.data_ptr(), K, args,
                                 d_list + 4 * f0, Dm.data_ptr(), Im.data_ptr())
        own.synchronize()
    t["tie"] = time.time() - t0
    return t, nf


def main():
    nq = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    dev = torch.device("cuda", 0)
    base = synth.sift_like(N, d=D, seed=1234)
    q = synth.sift_like(nq, d=D, seed=4321)
    cc, _ = api.train_ivfpq(base[:NLIST * 64], NLIST, 16)
    args = api.SearchArgs(metric=api.METRIC_L2, nprobe=P, min_score=0.0, max_score=1e30)
    dq = torch.from_numpy(q).to(dev)
    dD = torch.empty((nq, K), dtype=torch.float32, device=dev)
    dI = torch.empty((nq, K), dtype=torch.int64, device=dev)
    bucket = max(1000, int(2.5 * N / NLIST))

    one = api.GammaHip(0)
    one.ivfflat_init(D, NLIST, api.METRIC_L2, bucket_init_size=bucket)
    one.ivfflat_set_trained(cc)
    one.raw_init(D)
    fill(one, base)

    def run_one():
        one.ivfflat_search_device(dq.data_ptr(), nq, K, args, dD.data_ptr(), dI.data_ptr())
        one.synchronize()
    sec1 = timed(run_one, calls)
    ref_D, ref_I = dD.cpu().numpy().copy(), dI.cpu().numpy().copy()
    print(json.dumps({"config": "one handle", "nq": nq, "ms_per_call": round(sec1 * 1e3, 3)}), flush=True)

    for W in (2, 4):
        for sharded in (False, True):
            grp = api.GammaHipGroup([0] * W)
            for m in grp.members:
                m.ivfflat_init(D, NLIST, api.METRIC_L2, bucket_init_size=bucket)
                m.ivfflat_set_trained(cc)
                m.raw_init(D)
            if sharded:
                grp.set_raw_placement(True)
            grp.set_owners(None)
            fill(grp, base, grp.members, sharded)

            def run_grp():
                grp.ivfflat_search_device(dq.data_ptr(), nq, K, args, dD.data_ptr(), dI.data_ptr())
            sec = timed(run_grp, calls)
            same = bool(np.array_equal(dI.cpu().numpy(), ref_I) and dD.cpu().numpy().tobytes() == ref_D.tobytes())
            ph, nf = phases(grp.members, dq, nq, args)      # (once warm: the group's calls above sized every workspace)
            ph, nf = phases(grp.members, dq, nq, args)
            tot = sum(ph.values())
            print(json.dumps({"config": "group of %d, rows %s" % (W, "sharded" if sharded else "replicated"), "nq": nq,
                              "ms_per_call": round(sec * 1e3, 3), "vs_one_handle": round(sec / sec1, 3),
                              "equals_one_handle": same, "flagged": nf,
                              "phase_ms": {k: round(v * 1e3, 3) for k, v in ph.items()},
                              "phase_share": {k: round(v / tot, 3) for k, v in ph.items()},
                              "note": "members share one GPU: no statement about scaling over xGMI"}), flush=True)
            grp.close()
    one.close()


if __name__ == "__main__":
    main()
