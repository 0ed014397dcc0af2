// gamma_index_ivfpq_rawshard_hip.cc -- "raw_placement": "sharded" for the HIPIVFPQ model: the ABI calls it needs beyond those
// of the replicated mirror (the group's raw placement switch and row routing, the raw store's clear, the switch that lets a
// narrow store take sharded rows), registered with
// gamma_index_ivfpq_hip.cc.  A translation unit of its own: builds of the plugin against a C ABI without those entries
// leave this file out, and HIPIVFPQ::Init then rejects the value.
#include "gamma_index_ivfpq_hip.h"

namespace tig_gamma {

namespace {
const HIPRawShardOps kRawShardOps = {gamma_hip_group_set_raw_placement, gamma_hip_group_raw_put, gamma_hip_raw_clear,
                                     gamma_hip_set_sparse_narrow_rows};
const int registered_rawshard = RegisterHIPRawShard(&kRawShardOps);
}  // namespace

}  // namespace tig_gamma
