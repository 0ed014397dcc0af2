// gamma_index_ivfflat_sq8_hip.cc -- "raw_dtype": "sq8" for the HIPIVFFLAT model: the one ABI call it needs beyond those HIPIVFPQ's
// sq8 store registered (gamma_index_ivfpq_rawsq8_hip.cc) -- the handle's switch gamma_hip_set_ivfflat_sq8_rows -- registered with
// gamma_index_ivfpq_hip.cc.  A translation unit of its own: builds of the plugin against a C ABI without that entry leave this
// file out, and HIPIVFFLAT::Init then rejects the value.
#include "gamma_index_ivfpq_hip.h"

namespace tig_gamma {

namespace {
int IVFFlatSq8Rows(gamma_hip_index *h, int on) { return gamma_hip_set_ivfflat_sq8_rows(h, on); }
const int registered_ivfflat_sq8_rows = RegisterHIPIVFFlatSq8Rows(IVFFlatSq8Rows);
}  // namespace

}  // namespace tig_gamma
