// ivfflat_plan.cpp -- the host decisions of the IVFFLAT scan stage (ivfflat_plan.h).  Host code only.
#include "ivfflat_plan.h"

#include <stdlib.h>

namespace gh {

IvfflatSwitches IvfflatSwitches::from_env() {
    IvfflatSwitches s;
    s.no_lm = getenv("GAMMA_HIP_NO_IVFFLAT_LM") != nullptr;
    s.no_small_path = getenv("GAMMA_HIP_NO_SMALL_PATH") != nullptr;
    return s;
}

const IvfflatSwitches& IvfflatSwitches::get() {
    static const IvfflatSwitches s = from_env();
    return s;
}

bool ivfflat_lm_supported(int d) { return d == 16 || d == 32 || d == 64 || d == 96 || d == 128; }

int ivfflat_lm_shape(int d, int* kind, int* slab, int* qtile) {
    const int k = ivfflat_lm_supported(d) ? 1 : (d >= 16 && d <= 4096 && d % 16 == 0) ? 2 : 0;
    *kind = k;
    *slab = k == 1 ? d : k == 2 ? FS_SLAB : 0;
    *qtile = k == 1 ? FL_QT : k == 2 ? FS_QT : 0;
    return k;
}

int ivfflat_lm_tail_shape(int d, int elem_bytes, int* kind, int* load_bytes, int* qtile) {
    const int k = (d >= 1 && d <= 4096 && d % 16 != 0) ? 3 : 0;
    int lb = 16;   // gcd(16, d * elem_bytes)
    while (lb > 1 && ((int64_t)d * elem_bytes) % lb != 0) lb >>= 1;
    *kind = k;
    *load_bytes = lb;
    *qtile = FS_QT;
    return k;
}

size_t ivfflat_lm_scratch_bytes(int nq, int P, int nlist) { return ((size_t)nq * P + 4 * (size_t)nlist + 1) * sizeof(int); }

// Which scan runs over a chunk:
//
//                | single handle                                  | list shard
//   FILL         | never                                          | sparse_empty
//   LM_TAIL      | lm_tails, et <= 3, tail kind 3, pairs share    | never
//                | lists, no mask, !no_lm                         |
//   LM_FIXED /   | lm kind 1 / 2, pairs share lists, no mask,     | lm kind 1 / 2, pairs share lists, !no_lm; under a mask
//   LM_SLICED    | !no_lm (any et, sq8 included)                  | over the masked length table (masked_len)
//   PAIR         | everything else                                | everything else
//
// A single handle under a mask keeps the pair kernel: kept as found.
// A shard ignores lm_tails: the tail kernel has no sparse form, and the shard entry was left out when it was added.
IvfflatScanPlan ivfflat_scan_plan(const IvfflatScanShape& sh, const IvfflatSwitches& sw) {
    IvfflatScanPlan pl;
    if (sh.shard && sh.sparse_empty) {
        pl.kind = IvfflatScanPlan::FILL;
        return pl;
    }
    const bool lm_ok = !sw.no_lm && ivfflat_pairs_share_lists(sh.nc, sh.P, sh.nlist) && (sh.shard || !sh.masked);
    int kind = 0, a = 0, b = 0;   // (the tail form's kind does not depend on the element size)
    if (lm_ok && !sh.shard && sh.lm_tails && sh.et <= 3 && ivfflat_lm_tail_shape(sh.d, 1, &kind, &a, &b) == 3) {
        pl.kind = IvfflatScanPlan::LM_TAIL;
    } else if (lm_ok && ivfflat_lm_shape(sh.d, &kind, &a, &b) != 0) {
        pl.kind = kind == 1 ? IvfflatScanPlan::LM_FIXED : IvfflatScanPlan::LM_SLICED;
    } else {
        return pl;   // PAIR: no scratch
    }
    pl.scratch_bytes = ivfflat_lm_scratch_bytes(sh.nc, sh.P, sh.nlist);
    if (sh.shard) {   // room for the masked length table behind the scratch, mask or not
        pl.mlen_off = (pl.scratch_bytes + 15) & ~(size_t)15;
        pl.scratch_bytes = pl.mlen_off + (size_t)sh.nlist * sizeof(int);
        pl.masked_len = sh.masked;
    }
    return pl;
}

}  // namespace gh
