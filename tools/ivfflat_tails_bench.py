"""IVFFLAT search over row lengths that are no multiple of 16: the list-major scan (gamma_hip_set_ivfflat_lm_tails) against the
pair kernel on the same handle, ms per device-pointer call, one JSON line per (d, dtype, nq).

  python tools/ivfflat_tails_bench.py [--cases 100,200,300,1000,300:float16,100:uint8] [--neighbours 96,208,304,1008]
                                      [--nqs 256,1024,4096,16384] [--out FILE]

Per case one index, built as tools/ivfflat_dims_bench.py builds its indexes: 1 M rows for d <= 256, 200 k beyond, nlist 1024,
nprobe 16, k 10, L2.  A narrow store holds the rows rounded into its type (uint8: clipped to 0 .. 255).  Every batch size is
measured with the switch off and on, alternating, setting by setting: ms per call = the median of --reps repetitions of --calls
calls after a warm-up, with min - max.  The SHA-256 of the distances and labels of one call must be the same in both settings
(asserted).  `tails_faster_outside_both_spreads`: the switch-on call's slowest repetition beats the switch-off call's fastest.
--neighbours: the same measurement of multiples of 16 (fp32, the row-sliced or fixed-length kernel; the switch does not concern
them and stays off), for orientation."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from gamma_amd import api
from tools.ivfflat_dims_bench import K, NLIST, NPROBE, measure, rows_device

CASES = "100,200,300,1000,300:float16,100:uint8"
NEIGHBOURS = "96,208,304,1008"
NP = {"float32": np.float32, "float16": np.float16, "uint8": np.uint8}


def stored(x, dtype):
    """the rows as a store of `dtype` holds them, fp32"""
    if dtype == "uint8":
        x = np.clip(np.rint(x), 0, 255)
    return np.ascontiguousarray(x.astype(NP[dtype]).astype(np.float32))


def build(n, d, dtype):
    g = api.GammaHip(0)
    g.ivfflat_init(d, NLIST, api.METRIC_L2, bucket_init_size=max(1000, int(2.5 * n / NLIST)))
    cc, _ = g.kmeans(stored(rows_device(min(n, 64 * NLIST), d, 1234).cpu().numpy(), dtype), NLIST, 10)
    g.ivfflat_set_trained(cc)
    g.raw_init(d, dtype)
    for c in range(0, n, 65536):
        xb = stored(rows_device(min(65536, n - c), d, 1234, start=c).cpu().numpy(), dtype)
        g.raw_append(xb)
        g.add(xb, c)
    if dtype != "float32":
        g.set_ivfflat_narrow_rows(True)
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=CASES)
    ap.add_argument("--neighbours", default=NEIGHBOURS)
    ap.add_argument("--nqs", default="256,1024,4096,16384")
    ap.add_argument("--n-small", type=float, default=1e6)
    ap.add_argument("--n-big", type=float, default=2e5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    cases = [(int(c.split(":")[0]), (c.split(":") + ["float32"])[1], True) for c in a.cases.split(",") if c]
    cases += [(int(c), "float32", False) for c in a.neighbours.split(",") if c]
    bad = []
    for d, dtype, tail in cases:
        n = int(a.n_small if d <= 256 else a.n_big)
        g = build(n, d, dtype)
        try:
            for nq in [int(v) for v in a.nqs.split(",") if v]:
                res = dict(d=d, dtype=dtype, n=n, nq=nq, nlist=NLIST, nprobe=NPROBE, k=K, tail_length=tail,
                           tail_shape=list(api.ivfflat_lm_tail_shape(d, np.dtype(NP[dtype]).itemsize)))
                for on in ((False, True) if tail else (False,)):
                    g.set_ivfflat_lm_tails(on)
                    g.ivfflat_lm_tail_stats(reset=True)
                    r = measure(g, d, nq, api.METRIC_L2, a.reps, a.calls)
                    r["tail_chunks"] = g.ivfflat_lm_tail_stats()
                    res["tails_on" if on else "tails_off"] = r
                if tail:
                    off, on = res["tails_off"], res["tails_on"]
                    res["results_identical"] = bool(off["digest"] == on["digest"])
                    res["off_over_on"] = off["ms_per_call_median"] / on["ms_per_call_median"]
                    res["tails_faster_outside_both_spreads"] = bool(on["ms_max"] < off["ms_min"])
                    if not res["results_identical"]:
                        bad.append((d, dtype, nq))
                line = json.dumps(res)
                print(line, flush=True)
                if a.out:
                    with open(a.out, "a") as f:
                        f.write(line + "\n")
        finally:
            g.close()
        torch.cuda.empty_cache()
    assert not bad, "results differ between the two settings at (d, dtype, nq) = %s" % bad


if __name__ == "__main__":
    main()
