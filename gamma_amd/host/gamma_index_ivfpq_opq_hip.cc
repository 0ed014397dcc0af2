// gamma_index_ivfpq_opq_hip.cc -- "opq" for the HIPIVFPQ model: the entries of the C ABI that train, set, read and apply the
// rotation (gamma_hip_opq_*), registered with gamma_index_ivfpq_hip.cc as its OPQ ops table.  A translation unit of its own:
// builds of the plugin against a C ABI without those entries leave this file out, and HIPIVFPQ::Init then rejects "opq".
#include "gamma_index_ivfpq_hip.h"

namespace tig_gamma {

namespace {
const HIPOpqOps kOpqOps = {gamma_hip_opq_train, gamma_hip_opq_set, gamma_hip_opq_get, gamma_hip_opq_apply};
const int registered_opq = RegisterHIPOpq(&kOpqOps);
}  // namespace

}  // namespace tig_gamma
