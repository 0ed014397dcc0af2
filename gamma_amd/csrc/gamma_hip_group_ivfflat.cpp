// gamma_hip_group_ivfflat.cpp -- the entries of the C ABI behind the group's IVFFLAT search (gamma_hip_group_ivfflat_search*,
// gamma_hip_group.cpp): the single-handle device search and the list-shard building blocks of
// gamma_hip_search_ivfflat_shard.cpp.  gamma_hip_group.cpp is also built against a CPU stub of the ABI that has none of them
// (gamma_hip_group_ext.h), so it reaches them through the table registered here at static-initialisation time.
#include "../../include/gamma_hip.h"
#include "gamma_hip_group_ext.h"

namespace {

const gamma_group_ext::IvfflatOps kIvfflatOps = {
    gamma_hip_ivfflat_search_device, gamma_hip_ivfflat_coarse_device, gamma_hip_ivfflat_search_shard,
    gamma_hip_ivfflat_shard_export_rows, gamma_hip_ivfflat_shard_export, gamma_hip_ivfflat_merge, gamma_hip_ivfflat_merge_replay,
};
const int kRegistered = gamma_group_ext::register_ivfflat_ops(&kIvfflatOps);

}  // namespace
