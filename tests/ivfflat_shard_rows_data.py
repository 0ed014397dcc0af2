"""Data of the tests of the IVFFLAT list shards over float16 / uint8 / int8 rows (tests/test_gpu_ivfflat_shard_rows.py,
tests/test_gpu_group_ivfflat_rows.py, tests/test_ivfflat_shard_rows_cpu.py): which cases the GPU tests run,
the cross-shard tie case of every element type, and the stores' acceptance predicates restated for the CPU.

A case has `base` (what a caller hands to a store of the type) and `W` = base.astype(T).astype(float32) (what the store holds,
tests/ivfflat_rows_data.py); the oracle holds W.  The float16 rows round, so W != base."""
import ctypes as C

import numpy as np

from gamma_amd import _lib
from oracle import binding as B
from tests import ivfflat_lm_data as LM
from tests import ivfflat_rows_data as R
from tests import ivfflat_shard_ref as SR

L2, IP = B.METRIC_L2, B.METRIC_IP
DTYPES = R.DTYPES
K, P = 10, 4
# (d, metric, W): d 16 / 128 the fixed list-major kernel (16: the smallest row, 16 bytes of uint8), 144 the row-sliced one (one
# 128 slab plus one 16 piece), 24 / 20 the pair kernel (20: a byte row aligned to 4 bytes only)
SHAPES = [(16, L2, 2), (128, IP, 3), (144, L2, 4), (24, IP, 2), (20, L2, 3)]
SMALL, PAIR, FIXED, SLICED = 0, 1, 2, 3      # ivfflat_scan_stats
LM_STAT = {16: FIXED, 128: FIXED, 144: SLICED, 24: PAIR, 20: PAIR}
TIE_SHAPES = [(L2, 2), (IP, 3)]
TIE_SEED = {"float16": 3, "uint8": 3, "int8": 3}      # examined by tests/test_ivfflat_shard_rows_cpu.py
FILTER_SEED, UPDATE_SEED = 71, 21

_cache = {}


def case(d, dtype, metric):
    key = ("case", d, dtype, metric)
    if key not in _cache:
        _cache[key] = LM.Case(d, dtype, metric, seed=60 + d)
    return _cache[key]


class TieCaseI8(LM.Case):
    """SR.TieCase's construction with rows in [-128, 127]: every distinct row TIE_COPIES times, every other copy at the row's
    second-nearest centroid, so that equal distances reach a query from lists of different owners"""

    def __init__(self, d=32, metric=L2, N=3000, nlist=16, nq=33, seed=0):
        super().__init__(d, "int8", metric, N=N, nlist=nlist, nq=nq, seed=seed, ties=True)
        W64, c64 = self.W.astype(np.float64), self.cc.astype(np.float64)
        dis = (W64 ** 2).sum(1)[:, None] - 2.0 * W64 @ c64.T + (c64 ** 2).sum(1)[None, :]
        near = np.argsort(dis, axis=1, kind="stable")[:, :2]
        seen = {}
        lno = np.empty(N, dtype=np.int64)
        for i in range(N):
            key = self.W[i].tobytes()
            n = seen.get(key, 0)
            seen[key] = n + 1
            lno[i] = near[i, n & 1]
        order = np.argsort(lno, kind="stable")
        self.lists = [order[lno[order] == l].astype(np.int64) for l in range(nlist)]
        self.o = B.OracleIVFPQ(d, nlist, 1, 8, metric)
        self.o.set_trained(self.cc, np.zeros((256, d), np.float32), None)
        for l, ids in enumerate(self.lists):
            if len(ids):
                assert self.o.add_keys(l, ids, np.zeros((len(ids), 1), np.uint8))
        self.o.set_raw(self.raw)


def tie_case(dtype, metric):
    """integers in [0, 255] (SR.TieCase: exact in uint8 and in float16) or in [-128, 127] (int8)"""
    key = ("tie", "int8" if dtype == "int8" else "u8", metric)
    if key not in _cache:
        seed = TIE_SEED[dtype]
        _cache[key] = TieCaseI8(metric=metric, seed=seed) if dtype == "int8" else SR.TieCase(metric=metric, seed=seed)
    return _cache[key]


def edge_case(dtype, seed=19):
    return LM.edge_case(dtype, seed=seed)


def filter_case(dtype):
    return LM.Case(144, dtype, L2, seed=FILTER_SEED)


def changed_row(c, dtype, src_vid):
    """a row a caller would write over another: row src_vid moved by one step in one element, inside the type's range; returns
    (what the caller hands over, what the store then holds)"""
    new = c.base[src_vid].copy()
    if dtype == "float16":
        new[1] += 0.3      # (does not survive the rounding unchanged)
    else:
        new[1] += 1.0 if new[1] < R.RANGE[dtype][1] else -1.0
    return new, R.widened(new[None], dtype)[0]


def storable(x, dtype):
    """the stores' acceptance predicates over the rows x: uint8 / int8 through the library's own host-side check
    (gamma_hip_raw_i8_check), float16 restated -- a finite value whose rounding to binary16 is finite"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if dtype == "float16":
        with np.errstate(over="ignore"):
            return bool(np.isfinite(x).all() and np.isfinite(x.astype(np.float16)).all())
    bad = C.c_int64(-1)
    rc = _lib.load().gamma_hip_raw_i8_check(x.ctypes.data_as(_lib.f32p), x.size, 1 if dtype == "int8" else 0, C.byref(bad))
    return rc == 0
