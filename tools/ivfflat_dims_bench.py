"""IVFFLAT search across row lengths and batch sizes: ms per device-pointer call, one JSON line per (d, nq) (DESIGN.md
section 22).

  python tools/ivfflat_dims_bench.py [--dims 128,256,768,1024] [--nqs 256,1024,4096,16384] [--metric l2|ip] [--out FILE]
                                     [--compare FILE] [--label NAME]

Per d one IVFFLAT index: 1 M rows for d <= 256, 200 k beyond (--n-small / --n-big), synth.sift_like_device rows up to d = 128,
synth.embedding_like_device rows above, drawn on the device block by block and added through the host; nlist 1024 (centroids:
10 k-means iterations over the first 64 nlist rows), nprobe 16, k 10.  ms per call = the median of --reps repetitions of --calls
calls after a warm-up of the shape, with min - max.  `digest` is the SHA-256 of the distances and labels of one call: --compare
FILE asserts, configuration by configuration, that it equals the digest in FILE (the lines another build of the library printed)
and says whether this run is faster or slower beyond both runs' min - max ranges.
The tool uses only entries every build of the library has; gamma_hip_ivfflat_lm_shape / _scan_stats are reported where the loaded
library has them (lm_shape, scan_stats: small-path calls, chunks of the pair kernel, of the fixed-length and of the row-sliced
list-major kernel, of ONE call), null otherwise."""
import argparse
import hashlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from gamma_amd import api, synth

DIMS = (128, 256, 768, 1024)
NQS = (256, 1024, 4096, 16384)
NLIST, NPROBE, K = 1024, 16, 10


def rows_device(n, d, seed, start=0):
    if d <= 128:
        return synth.sift_like_device(n, d=d, seed=seed, start=start)
    return synth.embedding_like_device(n, d=d, seed=seed, start=start)


def build(n, d, metric):
    g = api.GammaHip(0)
    g.ivfflat_init(d, NLIST, metric, bucket_init_size=max(1000, int(2.5 * n / NLIST)))
    cc, _ = g.kmeans(rows_device(min(n, 64 * NLIST), d, 1234).cpu().numpy(), NLIST, 10)
    g.ivfflat_set_trained(cc)
    g.raw_init(d)
    step = 65536
    for c in range(0, n, step):
        xb = rows_device(min(step, n - c), d, 1234, start=c).cpu().numpy()
        g.raw_append(xb)
        g.add(xb, c)
    return g


def measure(g, d, nq, metric, reps, calls):
    dev = torch.device("cuda", 0)
    args = api.SearchArgs(metric=metric, nprobe=NPROBE, min_score=-3e38, max_score=3e38)
    dq = rows_device(2 * nq, d, 4321)
    D = torch.empty((nq, K), dtype=torch.float32, device=dev)
    I = torch.empty((nq, K), dtype=torch.int64, device=dev)
    run = lambda i: g.ivfflat_search_device(dq[(i % 2) * nq:].data_ptr(), nq, K, args, D.data_ptr(), I.data_ptr())
    run(0)
    run(1)
    g.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for i in range(calls):
            run(i)
        g.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0) / calls)
    stats = None
    if hasattr(g, "ivfflat_scan_stats"):
        g.ivfflat_scan_stats(reset=True)
    run(0)
    g.synchronize()
    if hasattr(g, "ivfflat_scan_stats"):
        stats = list(g.ivfflat_scan_stats())
    h = hashlib.sha256()
    h.update(D.cpu().numpy().tobytes())
    h.update(I.cpu().numpy().tobytes())
    med = float(np.median(ms))
    return dict(calls=calls, reps=reps, ms_per_call_median=med, ms_min=min(ms), ms_max=max(ms), queries_per_s=1e3 * nq / med,
                digest=h.hexdigest(), scan_stats=stats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default=",".join(str(d) for d in DIMS))
    ap.add_argument("--nqs", default=",".join(str(n) for n in NQS))
    ap.add_argument("--metric", default="l2", choices=["l2", "ip"])
    ap.add_argument("--n-small", type=float, default=1e6)
    ap.add_argument("--n-big", type=float, default=2e5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--compare", default="")
    a = ap.parse_args()
    metric = api.METRIC_L2 if a.metric == "l2" else api.METRIC_IP
    other = {}
    if a.compare:
        for line in open(a.compare):
            if line.strip():
                r = json.loads(line)
                other[(r["d"], r["n"], r["nq"], r["metric"])] = r
    shape_of = getattr(api, "ivfflat_lm_shape", None)
    bad = []
    for d in [int(v) for v in a.dims.split(",") if v]:
        n = int(a.n_small if d <= 256 else a.n_big)
        g = build(n, d, metric)
        try:
            for nq in [int(v) for v in a.nqs.split(",") if v]:
                res = dict(label=a.label, d=d, n=n, nq=nq, metric=a.metric, nlist=NLIST, nprobe=NPROBE, k=K)
                res.update(measure(g, d, nq, metric, a.reps, a.calls))
                res["lm_shape"] = list(shape_of(d)) if shape_of else None
                o = other.get((d, n, nq, a.metric))
                if o is not None:
                    res["same_results_as"] = o.get("label", "")
                    res["results_identical"] = bool(o["digest"] == res["digest"])
                    res["ms_vs_other"] = res["ms_per_call_median"] / o["ms_per_call_median"]
                    # faster (slower) when the two runs' min - max ranges do not overlap
                    res["faster_outside_both_spreads"] = bool(res["ms_max"] < o["ms_min"])
                    res["slower_outside_both_spreads"] = bool(res["ms_min"] > o["ms_max"])
                    if not res["results_identical"]:
                        bad.append((d, nq))
                line = json.dumps(res)
                print(line, flush=True)
                if a.out:
                    with open(a.out, "a") as f:
                        f.write(line + "\n")
        finally:
            g.close()
        torch.cuda.empty_cache()
    assert not bad, "results differ between the two builds at (d, nq) = %s" % bad


if __name__ == "__main__":
    main()
