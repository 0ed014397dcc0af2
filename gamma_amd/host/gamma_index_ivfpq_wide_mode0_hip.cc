// gamma_index_ivfpq_wide_mode0_hip.cc -- "pqwide_table_mode0": 1 for the HIPIVFPQ model with "nsubvector" beyond 64: the one ABI
// call it needs -- the handle's switch gamma_hip_ivfpq_wide_set_table_mode0, set before the lists initialiser -- registered with
// gamma_index_ivfpq_hip.cc.  A translation unit of its own: builds of the plugin against a C ABI without that entry leave
// this file out, and HIPIVFPQ::Init then rejects the key.
#include "gamma_index_ivfpq_hip.h"

namespace tig_gamma {

namespace {
int WideMode0Set(gamma_hip_index *h, int on) { return gamma_hip_ivfpq_wide_set_table_mode0(h, on); }
const int registered_wide_mode0 = RegisterHIPWideMode0(WideMode0Set);
}  // namespace

}  // namespace tig_gamma
