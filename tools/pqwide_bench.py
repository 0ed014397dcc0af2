"""Wide 8-bit IVFPQ (gamma_hip_ivfpq_wide_init, pqwide.hip) on an embedding-shaped workload, beside the plain scan of an
M = 64 index over the same data as the yardstick for scan code-bytes per second and LDS gathers per second.

Workload W: 1 M x 768 clustered vectors, nlist 4096, nprobe 32, recall_num 200, re-rank, k = 10, 16384-query device-pointer
calls; legs M = 96 and M = 128 (wide) and M = 64 (ivfpq_init with GAMMA_HIP_NO_SCAN_BOUND=1: the plain, unbounded scan).
The legs' handles are built first, then their calls ALTERNATE step by step; per leg the wall time of a call and every stage's
time from the handle's device events (summed over the call's sub-batches), as median and [min, max], and recall@10 against flat for the first 1024 queries.

    python tools/pqwide_bench.py [--n 1000000] [--steps 8] [--warmup 2] [--out profiles/pqwide_w.json]
    --lm-scan            every wide leg twice on ONE handle, gamma_hip_ivfpq_wide_set_lm_scan off and on,
                         alternating call by call after both are warmed up; the two settings' last answers are compared
    --table-mode0        every wide leg twice: its handle (table mode 1) and a second handle over the SAME trained state created with
                         gamma_hip_ivfpq_wide_set_table_mode0 under a lowered precomputed_table_max_bytes (table mode 0, DESIGN.md
                         section 40), alternating call by call; each handle's device memory is reported
    --sweep NAME=a,b,c   every wide leg additionally once per value of the environment switch NAME, alternating per call
                         (a build with an experiment switch in its launcher; the committed library reads none)"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def clustered(n, d, seed, centers):
    rng = np.random.default_rng(seed)
    out = np.empty((n, d), np.float32)
    for i0 in range(0, n, 1 << 17):
        m = min(1 << 17, n - i0)
        out[i0:i0 + m] = centers[rng.integers(0, len(centers), m)] + 0.35 * rng.standard_normal((m, d), dtype=np.float32)
    return out


def build(a, M, base, trained=None):
    """trained: (cc, pq) of the leg's mode-1 handle -- the handle is made in table mode 0 over that state"""
    from gamma_amd import api
    wide = M > 64
    if not wide:
        os.environ["GAMMA_HIP_NO_SCAN_BOUND"] = "1"   # read when the handle is created
    g = api.GammaHip(0)
    os.environ.pop("GAMMA_HIP_NO_SCAN_BOUND", None)
    d = base.shape[1]
    bucket = max(1000, a.n // a.nlist)
    if trained:
        old = api.get_precomputed_table_max_bytes()
        api.set_precomputed_table_max_bytes(a.nlist * M * 1024 - 1)
        try:
            g.ivfpq_wide_init(d, a.nlist, M, api.METRIC_L2, bucket_init_size=bucket, table_mode0=True)
        finally:
            api.set_precomputed_table_max_bytes(old)
    elif wide:
        g.ivfpq_wide_init(d, a.nlist, M, api.METRIC_L2, bucket_init_size=bucket)
    else:
        g.ivfpq_init(d, a.nlist, M, 8, api.METRIC_L2, bucket_init_size=bucket)
    t0 = time.time()
    cc, pq = trained or g.ivfpq_train(base[:min(a.n, a.nlist * 40)], a.nlist, M)
    g.ivfpq_set_trained(cc, pq, None)
    g.raw_init(d)
    g.raw_append(base)
    for i0 in range(0, a.n, 1 << 18):
        g.add(base[i0:i0 + (1 << 18)], i0)
    return g, round(time.time() - t0, 1), (cc, pq)


def spread(v):
    return [round(float(np.median(v)), 1), round(float(min(v)), 1), round(float(max(v)), 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--nprobe", type=int, default=32)
    ap.add_argument("--recall-num", type=int, default=200)
    ap.add_argument("--nq", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--legs", default="96,128,64")
    ap.add_argument("--sweep", default="")
    ap.add_argument("--lm-scan", action="store_true")
    ap.add_argument("--table-mode0", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch

    from gamma_amd import api
    centers = np.random.default_rng(1).standard_normal((2048, a.d), dtype=np.float32)
    base = clustered(a.n, a.d, 2, centers)
    q = clustered(a.nq, a.d, 3, centers)
    k, nf = 10, min(1024, a.nq)
    args = api.SearchArgs(metric=api.METRIC_L2, nprobe=a.nprobe, recall_num=a.recall_num, has_rank=True,
                          min_score=-3e38, max_score=3e38)
    dx = torch.from_numpy(q).cuda()
    dD = torch.empty((a.nq, k), dtype=torch.float32, device="cuda")
    dI = torch.empty((a.nq, k), dtype=torch.int64, device="cuda")
    sw_name, sw_vals = (a.sweep.split("=")[0], a.sweep.split("=")[1].split(",")) if a.sweep else ("", [""])
    legs, flat_I = [], None
    for M in [int(x) for x in a.legs.split(",")]:
        g, t_build, trained = build(a, M, base)
        if flat_I is None:
            flat_I = g.flat_search(q[:nf], k, args)[1]
        for v in (sw_vals if M > 64 else [""]):
            for lm in ((0, 1) if a.lm_scan and M > 64 else (None,)):
                legs.append(dict(M=M, g=g, sw=v, lm=lm, build_s=t_build, wall=[], stages=[]))
        g.profile_enable(1)
        if a.table_mode0 and M > 64:
            g0, t_build, _ = build(a, M, base, trained)
            assert g0.use_precomputed_table() == 0
            legs.append(dict(M=M, g=g0, sw="", lm=None, build_s=t_build, wall=[], stages=[]))
            g0.profile_enable(1)

    def call(leg):
        if sw_name and leg["sw"] != "":
            os.environ[sw_name] = leg["sw"]
        if leg["lm"] is not None:
            leg["g"].ivfpq_wide_set_lm_scan(leg["lm"])
        leg["g"].profile_reset()
        t0 = time.perf_counter()
        leg["g"].ivfpq_search_device(dx.data_ptr(), a.nq, k, args, dD.data_ptr(), dI.data_ptr())
        leg["g"].synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        prof = leg["g"].profile()
        return wall, {n: v[0] * 1e3 for n, v in prof.items() if isinstance(v, (tuple, list)) and len(v) >= 2 and v[1]}
    for step in range(a.warmup + a.steps):
        for leg in legs:
            wall, st = call(leg)
            if step >= a.warmup:
                leg["wall"].append(wall)
                leg["stages"].append(st)
    res, last = [], {}
    for leg in legs:
        g, M = leg["g"], leg["M"]
        call(leg)
        I = dI.cpu().numpy()
        if leg["lm"] is not None:   # off, then on: equal bytes
            last.setdefault((M, leg["sw"]), []).append((dD.cpu().numpy().tobytes(), I.tobytes()))
        recall = float(np.mean([len(set(I[i].tolist()) & set(flat_I[i].tolist())) / float(k) for i in range(nf)]))
        sizes = np.array([g.list_size(l) for l in range(a.nlist)], np.int64)
        # (a call of several sub-batches leaves the last one's rows: the mean over the rows that are an assignment)
        ci = g.last_stages(a.nq, a.nprobe, a.recall_num)["coarse_idx"]
        ci = ci[((ci >= 0) & (ci < a.nlist)).all(axis=1)]
        scanned = float(sizes[ci].sum()) / max(1, len(ci)) * a.nq
        names = leg["stages"][0].keys()
        stage_us = {n: spread([s.get(n, 0.0) for s in leg["stages"]]) for n in names}
        scan_us = stage_us.get("scan", [0.0])[0]
        res.append({"M": M, "scan": "wide" if M > 64 else "plain (GAMMA_HIP_NO_SCAN_BOUND=1)", "switch": leg["sw"], "lm_scan": leg["lm"],
                    "table_mode": g.use_precomputed_table(), "device_mem_bytes": g.total_mem_bytes(),
                    "lm_stats": list(g.ivfpq_wide_lm_stats()) if leg["lm"] else None,
                    "build_s": leg["build_s"], "wall_ms": spread(leg["wall"]), "qps": round(a.nq / (np.median(leg["wall"]) * 1e-3)),
                    "stage_us": stage_us, "codes_per_query": round(scanned / a.nq, 1), "max_list": int(sizes.max()),
                    "scan_code_bytes_per_s": float("%.4g" % (scanned * M / (scan_us * 1e-6))) if scan_us else None,
                    "scan_gathers_per_s": float("%.4g" % (scanned * M / (scan_us * 1e-6))) if scan_us else None,
                    "recall_at_10_vs_flat": round(recall, 4), "recall_queries": nf, "ties_not_honoured": g.ties_not_honoured()})
    out = {"workload": {k_: getattr(a, k_) for k_ in ("n", "d", "nlist", "nprobe", "recall_num", "nq", "steps", "warmup")},
           "sweep": sw_name, "lm_scan_equal_bytes": all(v[0] == v[1] for v in last.values()) if last else None, "legs": res}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    for g in {id(leg["g"]): leg["g"] for leg in legs}.values():
        g.close()


if __name__ == "__main__":
    main()
