"""IVFFLAT search over float16 / uint8 / int8 rows against the fp32 store: same lists, same store contents, one process
(DESIGN.md section 16).

  python tools/ivfflat_rows_bench.py [--shape lm|pair|all] [--n 1000000] [--out profiles/ivfflat_rows_{shape}.json]

The index is the README's IVFFLAT shape: n x 128 (min(rint(synth.sift_like / 2), 127): integer values in [0, 127], which float16,
uint8 AND int8 hold, so one base serves the four stores), nlist 4096, nprobe 32, k 10, L2.  The fp32 handle assigns the vectors;
the other three get its lists.  The results of the four must be identical: asserted.
lm  : 4096-query device-pointer calls -- the list-major kernel (k_ivfflat_lm).
pair: 64-query calls -- the small path, one workgroup per (query, probe) pair (k_ivfflat_scan).
Per store: ms per call (median of --reps repetitions of --calls calls, min - max), queries/s, the store's bytes.  The yardstick is
the fp32 store of the same process: per narrow type the ratio of medians and whether the narrow median lies inside the fp32
repetitions' own min - max spread or below it ("not slower").  One JSON line per shape."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from gamma_amd import api, synth

D, K, NPROBE = 128, 10, 32
SHAPES = {"lm": 4096, "pair": 64}
DTYPES = ("float32", "float16", "uint8", "int8")


def rows(n, seed):
    return np.minimum(np.rint(synth.sift_like(n, d=D, seed=seed) * np.float32(0.5)), np.float32(127.0)).astype(np.float32)


def build(base, cc, nlist, dtype, lists):
    """lists: None -- the handle assigns the vectors itself; else (list numbers, counts, vids) of the handle that did"""
    g = api.GammaHip(0)
    g.ivfflat_init(D, nlist, api.METRIC_L2, bucket_init_size=max(1000, int(2.5 * len(base) / nlist)))
    g.ivfflat_set_trained(cc)
    g.raw_init(D, dtype)
    if dtype != "float32":
        g.set_ivfflat_narrow_rows(True)
    for c in range(0, len(base), 1 << 16):
        xb = base[c:c + (1 << 16)]
        g.raw_append(xb)
        if lists is None:
            g.add(xb, c)
    if lists is not None:
        g.add_keys_batch(lists[0], lists[1], lists[2], np.zeros((len(lists[2]), 1), np.uint8))
    return g


def lists_of(g, nlist):
    nos, counts, vids = [], [], []
    for l in range(nlist):
        ids = g.get_list(l)[0]
        if len(ids):
            nos.append(l)
            counts.append(len(ids))
            vids.append(ids)
    return nos, counts, np.concatenate(vids)


def measure(g, q, nq, reps, calls):
    dev = torch.device("cuda", 0)
    args = api.SearchArgs(metric=api.METRIC_L2, nprobe=NPROBE, min_score=-3e38, max_score=3e38)
    dq = torch.from_numpy(q).to(dev)
    Dd = torch.empty((nq, K), dtype=torch.float32, device=dev)
    Id = torch.empty((nq, K), dtype=torch.int64, device=dev)
    run = lambda i: g.ivfflat_search_device(dq[(i % 2) * nq:].data_ptr(), nq, K, args, Dd.data_ptr(), Id.data_ptr())
    for i in range(2):
        run(i)
    g.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for i in range(calls):
            run(i)
        g.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0) / calls)
    run(0)
    g.synchronize()
    first = (Dd.cpu().numpy().copy(), Id.cpu().numpy().copy())
    st = g.raw_stats()
    med = float(np.median(ms))
    out = dict(ms_per_call_median=med, ms_min=min(ms), ms_max=max(ms), qps_median=nq / med * 1e3, raw_elem_bytes=g.raw_elem_bytes(),
               raw_elem_type=g.raw_elem_type(), raw_rows_bytes=st["rows"] * D * g.raw_elem_bytes(),
               total_mem_bytes=g.total_mem_bytes())
    return out, first


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES) + ["all"], default="all")
    ap.add_argument("--n", type=float, default=1e6)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--out", default="", help="file of the JSON line; {shape} is replaced")
    a = ap.parse_args()
    n, nlist = int(a.n), a.nlist
    shapes = sorted(SHAPES) if a.shape == "all" else [a.shape]
    t0 = time.time()
    base = rows(n, 1234)
    q = rows(2 * max(SHAPES.values()), 4321)
    cc, _ = api.train_ivfpq(base[:nlist * 64], nlist, 16)
    handles = {}
    try:
        lists = None
        for dtype in DTYPES:
            handles[dtype] = build(base, cc, nlist, dtype, lists)
            if lists is None:
                lists = lists_of(handles[dtype], nlist)
        build_s = round(time.time() - t0, 1)
        ok = True
        for shape in shapes:
            nq = SHAPES[shape]
            res = dict(shape=shape, n=n, d=D, nlist=nlist, nprobe=NPROBE, k=K, nq_call=nq, metric="L2", calls=a.calls, reps=a.reps,
                       build_s=build_s)
            firsts = {}
            for dtype in DTYPES:
                res[dtype], firsts[dtype] = measure(handles[dtype], q[:2 * nq], nq, a.reps, a.calls)
            f32 = res["float32"]
            for t in DTYPES[1:]:
                res[t]["ms_vs_float32"] = res[t]["ms_per_call_median"] / f32["ms_per_call_median"]
                res[t]["not_slower_than_float32_spread"] = bool(res[t]["ms_per_call_median"] <= f32["ms_max"])
            D32, I32 = firsts["float32"]
            same = all(firsts[t][0].tobytes() == D32.tobytes() and firsts[t][1].tobytes() == I32.tobytes() for t in DTYPES[1:])
            res["results_identical"] = bool(same)
            ok = ok and same
            line = json.dumps(res)
            print(line, flush=True)
            if a.out:
                with open(a.out.replace("{shape}", shape), "w") as f:
                    f.write(line + "\n")
    finally:
        for g in handles.values():
            g.close()
    assert ok, "narrow rows widen exactly: the four stores must give identical results"


if __name__ == "__main__":
    main()
