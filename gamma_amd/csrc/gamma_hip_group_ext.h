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
    // narrow rows sharded with their lists (gamma_hip_set_sparse_narrow_rows): the members convert, the group only asks
    int (*rows_check)(gamma_hip_index*, int64_t n, const float* vecs);   // the store's acceptance predicate over n rows, nothing written
    int (*same_rows)(gamma_hip_index*, gamma_hip_index*);                // 1: one element type, row length and sq8 ranges
};
int register_raw_ops(const RawOps* ops);   // returns 1 (a value for a static initialiser)

// What tells a handle that a group owns it: such a handle refuses an OPQ matrix (gamma_hip_opq_set; the group rotates nothing).
// Registered by the translation unit that defines gamma_hip_opq_set (gamma_hip_opq.cpp), so every library that can set a matrix
// also marks its group members -- independent of the raw-shard table above.  The CPU stub of the sanitizer builds has neither.
typedef int (*MemberMarkFn)(gamma_hip_index*);
int register_member_mark(MemberMarkFn fn);   // returns 1

// A family of members as the group's search sees it (gamma_hip_group.cpp runs ONE list-sharded protocol for all of them): the
// single-handle device search (replicated lists), the list-shard building blocks, and what only some families have.  The
// entries carry the superset of the families' arguments, in the order of the IVFPQ entries of include/gamma_hip.h; a family
// that has no use for one (the bound and its reduction, the coarse distances of the tie inputs, the query slice of the merge)
// registers an adapter that drops it.  The IVFPQ table is built inside gamma_hip_group.cpp from the ABI the stub has.  The
// IVFFLAT entries the stub does not have: their table is registered at static-initialisation time by
// gamma_hip_group_ivfflat.cpp; without it the group's IVFFLAT search answers GAMMA_HIP_EUNSUPPORTED with a message.
struct ShardFamily {
    const char* name;   // what the call's own messages begin with
    int (*search_device)(gamma_hip_index*, const gamma_hip_search_params*, int nq, const float* d_x, int k, float* d_D, int64_t* d_I);
    int (*coarse_device)(gamma_hip_index*, const gamma_hip_search_params*, int nq, const float* d_x, float* d_coarse_dis, int32_t* d_probe);
    // the scan of the owned probed lists: [nq][R] candidates of the whole batch (d_bound, reduce, user: bounded_scan only)
    int (*scan)(gamma_hip_index*, const gamma_hip_search_params*, int nq, const float* d_x, const float* d_coarse_dis, const int32_t* d_probe,
                int k, float* d_dis, int64_t* d_ids, float* d_bound, gamma_hip_bound_reduce_fn reduce, void* user);
    int (*shard_export_rows)(gamma_hip_index*, const gamma_hip_search_params*, int nf, const int32_t* d_probe_f, int64_t* max_entries);
    int (*shard_export)(gamma_hip_index*, const gamma_hip_search_params*, int nf, const float* d_xf, const float* d_cdis_f,
                        const int32_t* d_probe_f, int64_t stride, float* d_vals, int64_t* d_ids, int32_t* d_off);   // d_cdis_f: tie_coarse_dis only
    int (*merge)(gamma_hip_index*, const gamma_hip_search_params*, int nshards, int nq, const float* d_x_slice, int k, const float* d_all_dis,
                 const int64_t* d_all_ids, int q0, int nq_local, float* d_D, int64_t* d_I);
    int (*merge_replay)(gamma_hip_index*, const gamma_hip_search_params*, int nshards, int nf, const float* d_x_slice, int64_t stride,
                        const float* d_vals_all, const int64_t* d_ids_all, const int32_t* d_off_all, int k, const int32_t* d_list, float* d_D,
                        int64_t* d_I);
    bool wide_tables;      // the candidate tables are max(recall_num, k) wide (re-rank at the owner); otherwise k
    bool bounded_scan;     // the scan reduces one bound per query over the members: one more meeting point of the call
    bool tie_coarse_dis;   // the tie phase's export reads the flagged queries' coarse distances as well
    bool raw_rows;         // raw rows may be sharded with the lists: exact distances travel with candidates and exports
    bool rccl;             // RCCL may carry the exchanges; otherwise peer copies whatever the group's transport setting says
};
int register_ivfflat_ops(const ShardFamily* family);   // returns 1

int set_raw_sharded(gamma_hip_group* g, int sharded);
int raw_sharded(const gamma_hip_group* g);
int raw_put(gamma_hip_group* g, int64_t n, const int64_t* vids, const float* vecs, int64_t* n_skipped);

}  // namespace gamma_group_ext
