// gamma_index_ivfpq4_lm_hip.cc -- "pq4_lm_scan": 1 for the HIPIVFPQ model with "nbits_per_idx": 4: the two ABI calls it needs --
// the handle's switch gamma_hip_ivfpq4_set_lm_scan and the counters gamma_hip_ivfpq4_lm_stats -- registered with
// gamma_index_ivfpq_hip.cc.  A translation unit of its own: builds of the plugin against a C ABI without those entries leave
// this file out, and HIPIVFPQ::Init then rejects the key.
#include "gamma_index_ivfpq_hip.h"

namespace tig_gamma {

namespace {
int Pq4LmSet(gamma_hip_index *h, int on) { return gamma_hip_ivfpq4_set_lm_scan(h, on); }
int Pq4LmStats(gamma_hip_index *h, int64_t *calls, int64_t *units, int64_t *pairs) {
  return gamma_hip_ivfpq4_lm_stats(h, calls, units, pairs);
}
const HIPPq4LmOps pq4_lm_ops = {Pq4LmSet, Pq4LmStats};
const int registered_pq4_lm = RegisterHIPPq4Lm(&pq4_lm_ops);
}  // namespace

}  // namespace tig_gamma
