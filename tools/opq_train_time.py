"""Times gamma_hip_opq_train on Gaussian data of decaying variance: d = 128 / M 16 with the full 50 alternations, d = 768 /
M 64 with `--alt768` alternations (the polar factor's Jacobi sweeps run on one host thread and dominate there), 65536
points each.  Prints one line per shape; needs an MI355X.

    python tools/opq_train_time.py [--alt768 2]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alt768", type=int, default=2)
    a = ap.parse_args()
    from gamma_amd import api
    for d, M, niter in ((128, 16, 50), (768, 64, a.alt768)):
        rng = np.random.default_rng(d)
        x = (rng.standard_normal((65536, d)) * (0.99 ** np.arange(d))[None, :]).astype(np.float32)
        g = api.GammaHip(0)
        try:
            g.opq_train(x[:4096], M, 1)   # warm-up: code objects, allocator
            t = time.time()
            A, obj = g.opq_train(x, M, niter)
            dt = time.time() - t
            print("opq_train d=%d M=%d n=65536 alternations=%d: %.2f s (%.2f s per alternation), objective %.5g"
                  % (d, M, niter, dt, dt / niter, obj), flush=True)
        finally:
            g.close()


if __name__ == "__main__":
    main()
