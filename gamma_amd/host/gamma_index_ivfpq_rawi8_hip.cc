// gamma_index_ivfpq_rawi8_hip.cc -- "raw_dtype": "uint8" | "int8" for the HIPIVFPQ model: the ABI calls it needs beyond those of
// the fp32 mirror -- gamma_hip_raw_init_i8 and the writers' acceptance predicate gamma_hip_raw_i8_check -- registered with
// gamma_index_ivfpq_hip.cc.  A translation unit of its own: builds of the plugin against a C ABI without those entries leave
// this file out, and HIPIVFPQ::Init then rejects the two values.
#include "gamma_index_ivfpq_hip.h"

namespace tig_gamma {

namespace {
const HIPRawI8Ops kOps = {gamma_hip_raw_init_i8, gamma_hip_raw_i8_check};
const int registered_raw_i8 = RegisterHIPRawI8(&kOps);
}  // namespace

}  // namespace tig_gamma
