// gamma_index_ivfflat_group_hip.cc -- "devices" with several entries for the HIPIVFFLAT model: the one ABI call it needs beyond those
// HIPIVFPQ's group already uses -- gamma_hip_group_ivfflat_search -- registered with gamma_index_ivfpq_hip.cc.  A translation unit of
// its own: builds of the plugin against a C ABI without that entry leave this file out, and HIPIVFFLAT then opens one handle.
#include "gamma_index_ivfpq_hip.h"

namespace tig_gamma {

namespace {
int IVFFlatGroupSearch(gamma_hip_group *g, const gamma_hip_search_params *p, int nq, const float *x, int k, float *distances,
                       int64_t *labels) {
  return gamma_hip_group_ivfflat_search(g, p, nq, x, k, distances, labels);
}
const int registered_ivfflat_group = RegisterHIPIVFFlatGroup(IVFFlatGroupSearch);
}  // namespace

}  // namespace tig_gamma
