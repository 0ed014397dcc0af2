// gamma_hip_group_ext.h -- the seam between gamma_hip_group.cpp and gamma_hip_group_rawshard.cpp.
//
// gamma_hip_group.cpp is built in two settings: into libgamma_hip.so, and -- by the sanitizer builds of the tests -- against a
// CPU stub of the C ABI that predates the sparse raw store's drop / count entries.  It therefore names none of them: the
// entries the sharded raw placement needs reach it through the table below, registered at static-initialisation time by
// gamma_hip_group_rawshard.cpp, which also defines the public gamma_hip_group_*raw* entries on top of the functions declared
// here.  A build without that file has no table, and the sharded raw placement is refused with a message.
#pragma once
#include <stdint.h>

#include "../../include/gamma_hip.h"

namespace gamma_group_ext {

struct RawOps {
    int (*raw_drop)(gamma_hip_index*, int64_t, const int64_t*);
    int64_t (*raw_count)(gamma_hip_index*);
    int (*raw_clear)(gamma_hip_index*);
};
int register_raw_ops(const RawOps* ops);   // returns 1 (a value for a static initialiser)

// What tells a handle that a group owns it: such a handle refuses an OPQ matrix (gamma_hip_opq_set; the group rotates nothing).
// Registered by the translation unit that defines gamma_hip_opq_set (gamma_hip_opq.cpp), so every library that can set a matrix
// also marks its group members -- independent of the raw-shard table above.  The CPU stub of the sanitizer builds has neither.
typedef int (*MemberMarkFn)(gamma_hip_index*);
int register_member_mark(MemberMarkFn fn);   // returns 1

// The IVFFLAT search of the group (gamma_hip_group_ivfflat_search*, defined in gamma_hip_group.cpp) runs on entries the stub
// does not have either: the single-handle device search (replicated lists) and the list-shard building blocks.  Registered at
// static-initialisation time by gamma_hip_group_ivfflat.cpp; without the table the group's IVFFLAT search answers
// GAMMA_HIP_EUNSUPPORTED with a message.
struct IvfflatOps {
    int (*search_device)(gamma_hip_index*, const gamma_hip_search_params*, int, const float*, int, float*, int64_t*);
    int (*coarse_device)(gamma_hip_index*, const gamma_hip_search_params*, int, const float*, float*, int32_t*);
    int (*search_shard)(gamma_hip_index*, const gamma_hip_search_params*, int, const float*, const float*, const int32_t*, int, float*,
                        int64_t*);
    int (*shard_export_rows)(gamma_hip_index*, const gamma_hip_search_params*, int, const int32_t*, int64_t*);
    int (*shard_export)(gamma_hip_index*, const gamma_hip_search_params*, int, const float*, const int32_t*, int64_t, float*, int64_t*,
                        int32_t*);
    int (*merge)(gamma_hip_index*, const gamma_hip_search_params*, int, int, int, const float*, const int64_t*, int, int, float*,
                 int64_t*);
    int (*merge_replay)(gamma_hip_index*, const gamma_hip_search_params*, int, int, const float*, int64_t, const float*, const int64_t*,
                        const int32_t*, int, const int32_t*, float*, int64_t*);
};
int register_ivfflat_ops(const IvfflatOps* ops);   // returns 1

int set_raw_sharded(gamma_hip_group* g, int sharded);
int raw_sharded(const gamma_hip_group* g);
int raw_put(gamma_hip_group* g, int64_t n, const int64_t* vids, const float* vecs, int64_t* n_skipped);

}  // namespace gamma_group_ext
