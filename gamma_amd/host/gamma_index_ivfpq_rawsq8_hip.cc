// gamma_index_ivfpq_rawsq8_hip.cc -- "raw_dtype": "sq8" for the HIPIVFPQ model: the ABI calls it needs beyond those of the fp32
// mirror -- gamma_hip_raw_init_sq8, the ranges (gamma_hip_raw_sq8_set_ranges / _get_ranges / _train) and the writers' acceptance
// predicate gamma_hip_raw_sq8_check -- registered with gamma_index_ivfpq_hip.cc.  A translation unit of its own: builds of the
// plugin against a C ABI without those entries leave this file out, and HIPIVFPQ::Init then rejects the value.
#include "gamma_index_ivfpq_hip.h"

namespace tig_gamma {

namespace {
const HIPRawSq8Ops kOps = {gamma_hip_raw_init_sq8, gamma_hip_raw_sq8_set_ranges, gamma_hip_raw_sq8_get_ranges, gamma_hip_raw_sq8_train,
                           gamma_hip_raw_sq8_check};
const int registered_raw_sq8 = RegisterHIPRawSq8(&kOps);
}  // namespace

}  // namespace tig_gamma
