// gamma_index_binivf_lm_hip.cc -- "lm_scan": 1 for the HIPBINARYIVF model: the one ABI call it needs -- the handle's switch
// gamma_hip_binivf_set_lm_scan, at its measured default size -- registered with gamma_index_binivf_hip.cc.  A translation unit of
// its own: builds of the plugin against a C ABI without that entry leave this file out, and HIPBINARYIVF::Init then rejects
// the key.
#include "gamma_index_binivf_hip.h"

namespace tig_gamma {

namespace {
int BinaryIVFLmScanSet(gamma_hip_index *h, int on) { return gamma_hip_binivf_set_lm_scan(h, on, 0); }
const int registered_binivf_lm_scan = RegisterHIPBinaryIVFLmScan(BinaryIVFLmScanSet);
}  // namespace

}  // namespace tig_gamma
