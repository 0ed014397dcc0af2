"""Times gamma_hip_opq_apply_device (csrc/opq.hip) at the batch shapes DESIGN.md "OPQ" quotes and writes
profiles/opq_apply.json-shaped output: per shape the mean time of a call (device events around `reps` back-to-back
launches on the handle's stream, after a warm-up), the achieved fp32 FLOP rate (2 n d^2 per call) and the bytes a call
must move (n d read, n d written, d^2 matrix).  Needs an MI355X.

    python tools/opq_apply_bench.py [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    import torch

    from gamma_amd import api
    shapes = [(16384, 128, 16), (8192, 768, 64), (1, 128, 16), (1, 768, 64), (15, 15, 5)]   # (n, d, M); the last: the VALU chain
    rows = []
    for n, d, M in shapes:
        g = api.GammaHip(0)
        try:
            g.ivfpq_init(d, 16, M, 8, api.METRIC_L2)
            q, r = np.linalg.qr(np.random.default_rng(d).standard_normal((d, d)))
            g.opq_set(q.astype(np.float32))
            x = torch.randn(n, d, device="cuda")
            xt = torch.empty_like(x)
            s = torch.cuda.ExternalStream(g.stream())
            for _ in range(20):
                g.opq_apply_device(x.data_ptr(), n, xt.data_ptr())
            g.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(a.reps):
                g.opq_apply_device(x.data_ptr(), n, xt.data_ptr())
            e1.record(s)
            e1.synchronize()
            us = e0.elapsed_time(e1) * 1000.0 / a.reps
            flop = 2.0 * n * d * d
            rows.append(dict(n=n, d=d, kernel="k_opq_apply_mfma" if d % 4 == 0 else "k_opq_apply_valu", us_per_call=round(us, 2),
                             tflops=round(flop / us / 1e6, 2), min_bytes=4 * (2 * n * d + d * d), reps=a.reps))
            print(rows[-1], flush=True)
        finally:
            g.close()
    out = dict(what="gamma_hip_opq_apply_device: back-to-back launches on the handle's stream, device events, warm",
               device=torch.cuda.get_device_name(0), shapes=rows)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
