"""Flat search across row lengths: ms per 1024-query device-pointer call, one JSON line per shape.

  python tools/flat_dims_bench.py [--dims 24,65,96,...] [--out FILE] [--compare FILE] [--label NAME]

Per d: 1 M rows for d <= 1024, 262144 beyond (--n-small / --n-big); L2 over synth.sift_like_device rows up to d = 128, inner
product over synth.embedding_like_device rows above; 1024 queries, k = 100 (C2's call).  Rows are drawn on the device block by
block and appended through the host.  ms per call = the median of --reps repetitions of --calls calls after a warm-up of the
shape, with min - max; a shape whose warm-up call takes longer than --slow-ms (the exact vector kernel's shapes) is measured
with one call per repetition.  `digest` is the SHA-256 of the distances and labels of one call: --compare FILE asserts, shape
by shape, that it equals the digest in FILE (the lines another build of the library printed for the same shapes).
The tool uses only entries every build of the library has; gamma_hip_flat_filter_shape / _stats are reported where the loaded
library has them (filter_shape, filter_stats), null otherwise."""
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

DIMS = (24, 65, 96, 100, 128, 300, 320, 768, 1000, 1024, 1536, 1537, 2048, 3072, 4096)
NQ, K = 1024, 100


def rows_device(n, d, seed, start=0):
    if d <= 128:
        return synth.sift_like_device(n, d=d, seed=seed, start=start)
    return synth.embedding_like_device(n, d=d, seed=seed, start=start)


def build(n, d):
    g = api.GammaHip(0)
    g.raw_init(d)
    step = max(65536, (1 << 28) // (4 * d) // 65536 * 65536)      # ~256 MB per append, whole generator blocks
    for c in range(0, n, step):
        g.raw_append(rows_device(min(step, n - c), d, 1234, start=c).cpu().numpy())
    return g


def measure(g, d, reps, calls, slow_ms):
    dev = torch.device("cuda", 0)
    metric = api.METRIC_L2 if d <= 128 else api.METRIC_IP
    args = api.SearchArgs(metric=metric, min_score=-3e38, max_score=3e38)
    dq = rows_device(2 * NQ, d, 4321)
    D = torch.empty((NQ, K), dtype=torch.float32, device=dev)
    I = torch.empty((NQ, K), dtype=torch.int64, device=dev)
    run = lambda i: g.flat_search_device(dq[(i % 2) * NQ:].data_ptr(), NQ, K, args, D.data_ptr(), I.data_ptr())
    run(0)
    g.synchronize()
    t0 = time.perf_counter()
    run(1)
    g.synchronize()
    warm_ms = 1e3 * (time.perf_counter() - t0)
    if warm_ms > slow_ms:
        calls = 1
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for i in range(calls):
            run(i)
        g.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0) / calls)
    stats = None
    if hasattr(g, "flat_filter_stats"):
        g.flat_filter_stats(reset=True)
    run(0)
    g.synchronize()
    if hasattr(g, "flat_filter_stats"):
        stats = list(g.flat_filter_stats())
    h = hashlib.sha256()
    h.update(D.cpu().numpy().tobytes())
    h.update(I.cpu().numpy().tobytes())
    return dict(metric="L2" if metric == api.METRIC_L2 else "IP", calls=calls, reps=reps, ms_per_call_median=float(np.median(ms)),
                ms_min=min(ms), ms_max=max(ms), digest=h.hexdigest(), filter_stats=stats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default=",".join(str(d) for d in DIMS))
    ap.add_argument("--n-small", type=float, default=1e6)
    ap.add_argument("--n-big", type=float, default=262144)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--slow-ms", type=float, default=100.0)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--compare", default="")
    a = ap.parse_args()
    other = {}
    if a.compare:
        for line in open(a.compare):
            if line.strip():
                r = json.loads(line)
                other[(r["d"], r["n"])] = r
    shape_of = getattr(api, "flat_filter_shape", None)
    bad = []
    for d in [int(v) for v in a.dims.split(",") if v]:
        n = int(a.n_small if d <= 1024 else a.n_big)
        g = build(n, d)
        try:
            res = dict(label=a.label, d=d, n=n, nq_call=NQ, k=K)
            res.update(measure(g, d, a.reps, a.calls, a.slow_ms))
        finally:
            g.close()
        fs = shape_of(d) if shape_of else None
        res["filter_shape"] = list(fs) if fs else None
        o = other.get((d, n))
        if o is not None:
            res["same_results_as"] = o.get("label", "")
            res["results_identical"] = bool(o["digest"] == res["digest"])
            res["ms_vs_other"] = res["ms_per_call_median"] / o["ms_per_call_median"]
            # faster (slower) when the two runs' min - max ranges do not overlap
            res["faster_outside_both_spreads"] = bool(res["ms_max"] < o["ms_min"])
            res["slower_outside_both_spreads"] = bool(res["ms_min"] > o["ms_max"])
            if not res["results_identical"]:
                bad.append(d)
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        torch.cuda.empty_cache()
    assert not bad, "results differ between the two builds at d = %s" % bad


if __name__ == "__main__":
    main()
