// ivfflat_plan.h -- the host decisions of the IVFFLAT scan stage (gamma_hip_search_ivfflat.cpp ivfflat_scan_chunk) as plain values
// and pure functions: the environment switches (IvfflatSwitches), which list-major form a row length has (the shape functions),
// what a chunk looks like (IvfflatScanShape) and which scan runs over it (IvfflatScanPlan).  Nothing of HIP in here: a host
// compiler alone builds ivfflat_plan.cpp, and tests/ivfflat_plan_check.cc checks the table without a GPU.  ivfflat.hip takes
// its tile constants from here.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace gh {

constexpr int FL_QT = 32;      // fixed-length kernel (k_ivfflat_lm): queries per LDS tile
constexpr int FS_QT = 16;      // row-sliced kernels: queries per LDS tile = per work unit (their partial sums stay in registers)
constexpr int FS_SLAB = 128;   // row-sliced kernels: elements of a row a pair of threads holds at a time

// The switches of the stage, read from the environment once per process (get()).  This is the one place that reads them.
struct IvfflatSwitches {
    bool no_lm = false;           // GAMMA_HIP_NO_IVFFLAT_LM: the pair kernel where a list-major form would run
    bool no_small_path = false;   // GAMMA_HIP_NO_SMALL_PATH: the small-batch chains off (the IVFPQ and flat ones read it here too)
    static IvfflatSwitches from_env();
    static const IvfflatSwitches& get();
};

bool ivfflat_lm_supported(int d);
// the list-major form of rows of d floats: *kind 0 = none (the pair kernel), 1 = fixed-length (k_ivfflat_lm: the whole row in
// registers, d in {16, 32, 64, 96, 128}), 2 = row-sliced (k_ivfflat_lms: every other d % 16 == 0 up to 4096); *slab = the
// elements of a row a pair of threads holds at a time, *qtile = the queries per LDS tile (both 0 with kind 0).  Returns kind.
int ivfflat_lm_shape(int d, int* kind, int* slab, int* qtile);
// the list-major form of the lengths ivfflat_lm_shape answers 0 for: *kind 3 = row-sliced with the scanner's tail steps
// (k_ivfflat_lmt: 1 <= d <= 4096, d % 16 != 0), else 0; *load_bytes = gcd(16, d * elem_bytes), the alignment every row of such a
// store has and the width of the kernel's row loads; *qtile = the queries per LDS tile (k_ivfflat_lms's).  Returns kind.
int ivfflat_lm_tail_shape(int d, int elem_bytes, int* kind, int* load_bytes, int* qtile);
// scratch of a list-major launch: inv [nq * P] ints, then cnt | start | cur [nlist] ints each, ustart [nlist + 1]
size_t ivfflat_lm_scratch_bytes(int nq, int P, int nlist);

// enough (query, probe) pairs that lists are shared: a list's rows are worth reading once for all the queries probing it
inline bool ivfflat_pairs_share_lists(int64_t nq, int P, int nlist) { return nq * P >= 2 * (int64_t)nlist; }

struct IvfflatScanShape {
    int nc = 0, P = 0, nlist = 0, d = 0;
    int et = 0;                  // the store's element type (gamma_hip_raw_elem_type: 0 fp32, 1 float16, 2 uint8, 3 int8, 4 sq8)
    bool shard = false;          // the preassigned scan of a list shard (search_shard, shard_export); else the single handle's
    bool masked = false;         // the handle has a list mask
    bool sparse = false;         // the rows live in a sparse store (no kind depends on it: the launch takes the sparse body)
    bool sparse_empty = false;   // ... that never took a row
    bool lm_tails = false;       // gamma_hip_set_ivfflat_lm_tails
};

struct IvfflatScanPlan {
    // FILL: nothing is scanned, the slab gets the sentinel.  PAIR: one workgroup per (query, probe) pair (rerank.hip).
    // LM_FIXED / LM_SLICED / LM_TAIL: list-major, ivfflat_lm_shape's kind 1 / 2 and ivfflat_lm_tail_shape's kind 3 (ivfflat.hip).
    enum Kind { FILL, PAIR, LM_FIXED, LM_SLICED, LM_TAIL } kind = PAIR;
    bool masked_len = false;    // the kernels read a length table in which an unowned list is empty, at scratch + mlen_off
    size_t scratch_bytes = 0;   // of w_lm_units (0: the kind takes none)
    size_t mlen_off = 0;
};
IvfflatScanPlan ivfflat_scan_plan(const IvfflatScanShape& sh, const IvfflatSwitches& sw);

}  // namespace gh
