"""GPU: random binary IVF shapes, filters and score windows against the restatement (tests/binivf_ref.py), strictly.
Seeds: GAMMA_BINIVF_FUZZ_SEEDS (comma-separated; default a small fixed set)."""
import os

import numpy as np
import pytest

from gamma_amd import api
from tests import binivf_ref as BR

pytestmark = pytest.mark.gpu

SEEDS = [int(s) for s in os.environ.get("GAMMA_BINIVF_FUZZ_SEEDS", "1,2,3,4,5,6").split(",") if s.strip()]


@pytest.mark.parametrize("seed", SEEDS)
def test_binivf_fuzz(seed):
    rng = np.random.default_rng(seed)
    nbits = int(rng.choice([8, 16, 24, 40, 64, 128, 256, 320, 512]))
    nlist = int(rng.choice([1, 3, 8, 17, 64]))
    n = int(rng.integers(max(nlist, 50), 4000))
    base = BR.clustered_codes(n, nbits, int(rng.integers(1, 20)), flip=float(rng.choice([0.0, 0.02, 0.1])), seed=seed,
                              dup_frac=float(rng.choice([0.0, 0.3])))
    cc = base[rng.choice(n, nlist, replace=False)].copy()
    lists = BR.assign_lists(base, cc)
    g = api.GammaHip(0)
    try:
        g.binivf_init(nbits, nlist, bucket_init_size=int(rng.integers(1, 2000)))
        g.binivf_set_trained(cc)
        g.binivf_add(base, 0)
        deleted = rng.choice(n, int(rng.integers(0, n // 4 + 1)), replace=False)
        if deleted.size:
            g.bitmap_upload(np.zeros(n // 8 + 1, np.uint8), n)
            g.bitmap_set(deleted)
        x = np.concatenate([base[rng.integers(0, n, 10)], BR.clustered_codes(10, nbits, 3, seed=seed + 7)])
        for _ in range(4):
            k = int(rng.choice([1, 2, 5, 16, 63, 64, 65, 128, 257, 600]))
            nprobe = int(rng.integers(-1, nlist + 3))
            lo, hi = [(None, None), (0, 1e4), (float(rng.integers(0, 5)), float(rng.integers(5, nbits + 1)))][rng.integers(0, 3)]
            ranges = None
            if rng.random() < 0.5:
                ranges = [(rng.choice(n, int(rng.integers(0, n)), replace=False), bool(rng.random() < 0.5))]
            f = BR.Filter(deleted=deleted if deleted.size else None, ranges=ranges)
            rf = None if ranges is None else [api.make_range_filter(d, b_not_in=b) for d, b in ranges]
            D, I = g.binivf_search(x, k, api.SearchArgs(nprobe=nprobe, min_score=lo, max_score=hi, range_filters=rf))
            Dr, Ir = BR.search(lists, cc, x, k, nprobe, lo, hi, filt=f)
            assert np.array_equal(I, Ir) and D.tobytes() == Dr.tobytes(), (seed, nbits, nlist, k, nprobe, lo, hi)
    finally:
        g.close()
