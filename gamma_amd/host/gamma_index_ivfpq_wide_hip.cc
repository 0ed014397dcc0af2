// gamma_index_ivfpq_wide_hip.cc -- "nsubvector" 65 .. 256 at "nbits_per_idx": 8 for the HIPIVFPQ model: the one ABI call such an
// index needs beyond those of a narrower one, gamma_hip_ivfpq_wide_init, registered with gamma_index_ivfpq_hip.cc as the
// wide lists initialiser.  A translation unit of its own: builds of the plugin against a C ABI without that entry leave this
// file out, and HIPIVFPQ::Init then rejects the value as before.
#include "gamma_index_ivfpq_hip.h"

namespace tig_gamma {

namespace {
int InitListsWide(gamma_hip_index *h, int d, int nlist, int M, int metric, int bucket_init_size, int bucket_max_size) {
  return gamma_hip_ivfpq_wide_init(h, d, nlist, M, metric, bucket_init_size, bucket_max_size);
}
const int registered_lists_init_wide = RegisterHIPWideInit(InitListsWide);
}  // namespace

}  // namespace tig_gamma
