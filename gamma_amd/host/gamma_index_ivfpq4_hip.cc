// gamma_index_ivfpq4_hip.cc -- "nbits_per_idx": 4 for the HIPIVFPQ model: the one ABI call a 4-bit index needs beyond those
// of an 8-bit one, gamma_hip_ivfpq4_init, registered with gamma_index_ivfpq_hip.cc as the lists initialiser for nbits 4.
// A translation unit of its own: builds of the plugin against a C ABI without that entry leave this file out, and
// HIPIVFPQ::Init then rejects the value as before.
#include "gamma_index_ivfpq_hip.h"

namespace tig_gamma {

namespace {
int InitLists4(gamma_hip_index *h, int d, int nlist, int M, int metric, int bucket_init_size, int bucket_max_size) {
  return gamma_hip_ivfpq4_init(h, d, nlist, M, metric, bucket_init_size, bucket_max_size);
}
const int registered_lists_init4 = RegisterHIPListsInit(4, InitLists4);
}  // namespace

}  // namespace tig_gamma
