// gamma_index_ivfflat_tails_hip.cc -- "lm_tails": 1 for the HIPIVFFLAT model: the two ABI calls it needs -- the handle's switch
// gamma_hip_set_ivfflat_lm_tails and its counter gamma_hip_ivfflat_lm_tail_stats -- registered with gamma_index_ivfpq_hip.cc.  A
// translation unit of its own: builds of the plugin against a C ABI without those entries leave this file out, and
// HIPIVFFLAT::Init then rejects the key.
#include "gamma_index_ivfpq_hip.h"

namespace tig_gamma {

namespace {
int IVFFlatTailsSet(gamma_hip_index *h, int on) { return gamma_hip_set_ivfflat_lm_tails(h, on); }
int IVFFlatTailsStats(gamma_hip_index *h, int64_t *out1, int reset) { return gamma_hip_ivfflat_lm_tail_stats(h, out1, reset); }
const HIPIVFFlatTailsOps ivfflat_tails_ops = {IVFFlatTailsSet, IVFFlatTailsStats};
const int registered_ivfflat_tails = RegisterHIPIVFFlatTails(&ivfflat_tails_ops);
}  // namespace

}  // namespace tig_gamma
