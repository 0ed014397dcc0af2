// gamma_hip_group_ivfflat.cpp -- the IVFFLAT family of the group's search (gamma_group_ext::ShardFamily; the protocol itself is
// in gamma_hip_group.cpp): the single-handle device search and the list-shard building blocks of
// gamma_hip_search_ivfflat_shard.cpp.  gamma_hip_group.cpp is also built against a CPU stub of the ABI that has none of them
// (gamma_hip_group_ext.h), so it reaches them through the table registered here at static-initialisation time.  The table's
// entries take the arguments of the IVFPQ ones; the adapters drop what IVFFLAT has no use for.
#include "../../include/gamma_hip.h"
#include "gamma_hip_group_ext.h"

namespace {

int scan(gamma_hip_index* h, const gamma_hip_search_params* p, int nq, const float* d_x, const float* d_coarse_dis, const int32_t* d_probe, int k,
         float* d_dis, int64_t* d_ids, float*, gamma_hip_bound_reduce_fn, void*) {
    return gamma_hip_ivfflat_search_shard(h, p, nq, d_x, d_coarse_dis, d_probe, k, d_dis, d_ids);
}
int shard_export(gamma_hip_index* h, const gamma_hip_search_params* p, int nf, const float* d_xf, const float*, const int32_t* d_probe_f,
                 int64_t stride, float* d_vals, int64_t* d_ids, int32_t* d_off) {
    return gamma_hip_ivfflat_shard_export(h, p, nf, d_xf, d_probe_f, stride, d_vals, d_ids, d_off);
}
int merge(gamma_hip_index* h, const gamma_hip_search_params* p, int nshards, int nq, const float*, int k, const float* d_all_dis,
          const int64_t* d_all_ids, int q0, int nq_local, float* d_D, int64_t* d_I) {
    return gamma_hip_ivfflat_merge(h, p, nshards, nq, k, d_all_dis, d_all_ids, q0, nq_local, d_D, d_I);
}

const gamma_group_ext::ShardFamily kIvfflatFamily = {
    "ivfflat_search", gamma_hip_ivfflat_search_device, gamma_hip_ivfflat_coarse_device, scan, gamma_hip_ivfflat_shard_export_rows, shard_export,
    merge, gamma_hip_ivfflat_merge_replay,
    /*wide_tables*/ false, /*bounded_scan*/ false, /*tie_coarse_dis*/ false, /*raw_rows*/ false, /*rccl*/ false,
};
const int kRegistered = gamma_group_ext::register_ivfflat_ops(&kIvfflatFamily);

}  // namespace
