// gamma_index_ivfpq_rawf16_hip.cc -- "raw_dtype": "float16" for the HIPIVFPQ model: the one ABI call it needs beyond those of
// the fp32 mirror, gamma_hip_raw_init_f16, registered with gamma_index_ivfpq_hip.cc as the raw store's initialiser.  A
// translation unit of its own: builds of the plugin against a C ABI without that entry leave this file out, and
// HIPIVFPQ::Init then rejects the value.
#include "gamma_index_ivfpq_hip.h"

namespace tig_gamma {

namespace {
int RawInitF16(gamma_hip_index *h, int d) { return gamma_hip_raw_init_f16(h, d); }
const int registered_raw_init_f16 = RegisterHIPRawInitF16(RawInitF16);
}  // namespace

}  // namespace tig_gamma
