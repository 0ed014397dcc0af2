// gamma_index_ivfpq_wide_lm_hip.cc -- "pqwide_lm_scan": 1 for the HIPIVFPQ model with "nsubvector" beyond 64: the two ABI calls it
// needs -- the handle's switch gamma_hip_ivfpq_wide_set_lm_scan and the counters gamma_hip_ivfpq_wide_lm_stats -- registered with
// gamma_index_ivfpq_hip.cc.  A translation unit of its own: builds of the plugin against a C ABI without those entries leave
// this file out, and HIPIVFPQ::Init then rejects the key.
#include "gamma_index_ivfpq_hip.h"

namespace tig_gamma {

namespace {
int WideLmSet(gamma_hip_index *h, int on) { return gamma_hip_ivfpq_wide_set_lm_scan(h, on); }
int WideLmStats(gamma_hip_index *h, int64_t *calls, int64_t *units, int64_t *pairs) {
  return gamma_hip_ivfpq_wide_lm_stats(h, calls, units, pairs);
}
const HIPWideLmOps wide_lm_ops = {WideLmSet, WideLmStats};
const int registered_wide_lm = RegisterHIPWideLm(&wide_lm_ops);
}  // namespace

}  // namespace tig_gamma
