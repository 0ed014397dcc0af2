// gamma_index_ivfflat_group_rows_hip.cc -- "group_rows" for the HIPIVFFLAT model on several devices: "float32" (the default: the
// members hold fp32 rows, and a narrow raw_dtype beside several devices is rejected as it always was) | "raw_dtype" (the members
// hold their rows in raw_dtype -- float16 / uint8 / int8 -- and the group's IVFFLAT search reads them there: the shard entries
// serve a narrow store after gamma_hip_set_ivfflat_narrow_rows).  The key's parser and the decision, no device touched,
// registered with gamma_index_ivfpq_hip.cc.  A translation unit of its own: a build of the plugin without it never reads the key.
#include <strings.h>

#include <cstdio>

#include "gamma_index_ivfpq_hip.h"

namespace tig_gamma {

namespace {
#define GLOG(...)                                \
  do {                                           \
    fprintf(stderr, "[HIPIVFPQ] HIPIVFFLAT: ");  \
    fprintf(stderr, __VA_ARGS__);                \
    fprintf(stderr, "\n");                       \
  } while (0)

int IVFFlatGroupRows(const std::string &model_parameters, int et, size_t ndevices, bool device_filters, int *members_narrow) {
  *members_narrow = 0;
  utils::JsonParser jp;
  if (model_parameters == "" || jp.Parse(model_parameters.c_str()) || !jp.Contains("group_rows")) return 0;
  std::string v;
  const bool got = !jp.GetString("group_rows", v);
  if (got && !strcasecmp("float32", v.c_str())) return 0;
  if (!got || strcasecmp("raw_dtype", v.c_str())) {
    GLOG("invalid group_rows = %s (\"float32\" or \"raw_dtype\")", got ? v.c_str() : "(not a string)");
    return -2;
  }
  if (ndevices < 2) {
    GLOG("group_rows = raw_dtype needs several devices (one device holds its rows in raw_dtype anyway)");
    return -2;
  }
  if (et == 4) {
    GLOG("group_rows = raw_dtype with raw_dtype = sq8 is not supported (the trained ranges would have to reach every member)");
    return -2;
  }
  if (device_filters) {
    GLOG("group_rows = raw_dtype with device_filters is not supported (several devices: the columns live on one handle)");
    return -2;
  }
  *members_narrow = et >= 1 && et <= 3;   // (raw_dtype float32: accepted, and means nothing)
  return 0;
}
const int registered_ivfflat_group_rows = RegisterHIPIVFFlatGroupRows(IVFFlatGroupRows);
}  // namespace

}  // namespace tig_gamma
