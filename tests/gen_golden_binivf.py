"""Writes tests/golden/binivf_train.npz: the centroid codes IndexBinaryIVF::train's clustering gives on a few tie-heavy
code sets, computed by the compiled faiss of oracle/_ref (ref_kmeans on the codes' +-1 decoding, then real_to_binary).
Run from the repository root where oracle/_ref is built:  python -m tests.gen_golden_binivf"""
import os

import numpy as np

from oracle import binding as B
from tests import binivf_ref as BR

CASES = [  # (name, n, nbits, nlist, seed)
    ("b64_l16", 16 * 60, 64, 16, 11),
    ("b256_l16", 16 * 80, 256, 16, 12),
    ("b512_l16_eq", 16, 512, 16, 13),   # n == nlist: the copy path
    ("b256_l64", 64 * 50, 256, 64, 14),
]


def main():
    assert B.have_ref(), "oracle/_ref not built"
    out = {}
    for name, n, nbits, nlist, seed in CASES:
        codes = BR.clustered_codes(n, nbits, max(2, nlist // 2), flip=0.03, seed=seed, dup_frac=0.2)
        out[name + "_codes"] = codes
        out[name + "_cc"] = BR.train(codes, nlist, use_ref=True)
        out[name + "_nlist"] = np.int64(nlist)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "binivf_train.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
