// gamma_index_ivfflat_rows_hip.cc -- "raw_dtype": "float16" | "uint8" | "int8" for the HIPIVFFLAT model: the one ABI call it needs
// beyond those HIPIVFPQ's narrow stores registered -- the handle's switch gamma_hip_set_ivfflat_narrow_rows -- registered with
// gamma_index_ivfpq_hip.cc.  A translation unit of its own: builds of the plugin against a C ABI without that entry leave this
// file out, and HIPIVFFLAT::Init then rejects the three values.
#include "gamma_index_ivfpq_hip.h"

namespace tig_gamma {

namespace {
int IVFFlatNarrowRows(gamma_hip_index *h, int on) { return gamma_hip_set_ivfflat_narrow_rows(h, on); }
const int registered_ivfflat_rows = RegisterHIPIVFFlatRows(IVFFlatNarrowRows);
}  // namespace

}  // namespace tig_gamma
