"""The spread scan of the binary IVF model (gamma_amd/csrc/binivf_spread.hip) restated at the value level, over
tests/binivf_ref.py: a query's row sequence (its probed lists in coarse order, each list in list order), cut into chunks of
C rows that never span two lists; B_c = the k-th smallest valid distance of the rows before chunk c; the candidates are the
valid rows with dis < B_c.  Helpers of tests/test_binivf_spread_cpu.py and tests/test_gpu_binivf_spread.py."""
import numpy as np

from tests import binflat_ref as BF
from tests import binivf_ref as BR


def chunk_counts(lens, C):
    """chunks of every list of a probe sequence: ceil(len / C), 0 for an empty list or a -1 slot (len 0)"""
    return [(int(n) + C - 1) // C for n in lens]


def sequence(lists, probes, xq, C, lo=None, hi=None, filt=None):
    """One query over its probe row (list numbers, -1 = no centroid): (vals float32, ids int64, chunk int64) of the VALID
    rows in scan order, and the number of chunks and of rows scanned."""
    lo = np.float32(BR.FLT_TINY if lo is None else lo)
    hi = np.float32(BR.FLT_MAX if hi is None else hi)
    vals, ids, chunk = [], [], []
    nch = rows = 0
    for l in probes:
        if l < 0:
            continue
        lv, lc = lists[int(l)]
        if lv.size == 0:
            continue
        keep = lv >= 0
        if filt is not None:
            keep &= filt.valid(lv)
        dis = BR.hamming(xq, lc).astype(np.float32)
        keep &= (dis <= hi) & (dis >= lo)
        vals.append(dis[keep])
        ids.append(lv[keep])
        chunk.append(nch + np.nonzero(keep)[0] // C)
        nch += (lv.size + C - 1) // C
        rows += lv.size
    if not vals:
        return np.empty(0, np.float32), np.empty(0, np.int64), np.empty(0, np.int64), nch, rows
    return np.concatenate(vals), np.concatenate(ids), np.concatenate(chunk).astype(np.int64), nch, rows


def candidates(vals, chunk, k, nch):
    """bool per valid row: dis < B_(its chunk)"""
    if vals.size == 0:
        return np.zeros(0, bool)
    B = np.full(max(nch, 1), np.inf)
    for c in range(nch):
        pre = vals[chunk < c]
        if pre.size >= k:
            B[c] = np.partition(pre, k - 1)[k - 1]
    return vals < B[chunk]


def counts(lists, cc, x, k, nprobe, C, lo=None, hi=None, filt=None):
    """over the queries x: (heap admissions of the serial scan, candidates of the spread scan, chunks, valid rows)"""
    P = BR.resolve_nprobe(nprobe, cc.shape[0])
    _, probes = BR.coarse(x, cc, P)
    adm = cand = chunks = valid = 0
    for r in range(x.shape[0]):
        vals, _, chunk, nch, _ = sequence(lists, probes[r], x[r], C, lo, hi, filt)
        adm += int(BF.admitted(vals, k).sum())
        cand += int(candidates(vals, chunk, k, nch).sum())
        chunks += nch
        valid += int(vals.size)
    return adm, cand, chunks, valid
