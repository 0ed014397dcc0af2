// gamma_hip_group_rawshard.cpp -- raw vectors sharded with their lists in the in-process group: the public entries
// (include/gamma_hip.h, gamma_hip_group_set_raw_placement / _raw_placement / _raw_put) and the registration of the sparse
// store's entries the group's Update and placement switch call (gamma_hip_group_ext.h says why they go through a table).
#include "gamma_hip_group_ext.h"
#include "gamma_hip_internal.h"

namespace {
// (the two entries of the table that are no part of the C ABI: the store's internals, gamma_hip_internal.h)
int rows_check(gamma_hip_index* h, int64_t n, const float* vecs) { return ghi::raw_rows_check(h, n, vecs); }
int same_rows(gamma_hip_index* a, gamma_hip_index* b) { return ghi::raw_same_rows(a, b) ? 1 : 0; }
const gamma_group_ext::RawOps kOps = {gamma_hip_raw_drop, gamma_hip_raw_count, gamma_hip_raw_clear, rows_check, same_rows};
const int registered = gamma_group_ext::register_raw_ops(&kOps);
}  // namespace

extern "C" {

int gamma_hip_group_set_raw_placement(gamma_hip_group* g, int sharded) {
    (void)registered;
    return gamma_group_ext::set_raw_sharded(g, sharded);
}
int gamma_hip_group_raw_placement(const gamma_hip_group* g) { return gamma_group_ext::raw_sharded(g); }
int gamma_hip_group_raw_put(gamma_hip_group* g, int64_t n, const int64_t* vids, const float* vecs, int64_t* n_skipped) {
    return gamma_group_ext::raw_put(g, n, vids, vecs, n_skipped);
}

}  // extern "C"
