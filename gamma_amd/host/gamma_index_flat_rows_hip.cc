// gamma_index_flat_rows_hip.cc -- "raw_dtype": "float16" | "uint8" | "int8" for the HIPFLAT model: the one ABI call it needs
// beyond those HIPIVFPQ's narrow stores registered -- the handle's switch gamma_hip_set_flat_narrow_rows -- registered with
// gamma_index_flat_hip.cc.  A translation unit of its own: builds of the plugin against a C ABI without that entry leave this
// file out, and HIPFLAT::Init then rejects the three values.
#include "gamma_index_flat_hip.h"

namespace tig_gamma {

namespace {
int FlatNarrowRows(gamma_hip_index *h, int on) { return gamma_hip_set_flat_narrow_rows(h, on); }
const int registered_flat_rows = RegisterHIPFlatRows(FlatNarrowRows);
}  // namespace

}  // namespace tig_gamma
