// TEST INFRASTRUCTURE: a stand-in for the nine RCCL entries gamma_amd/csrc/gamma_hip_group.cpp resolves by name, so that the
// group's RCCL transport (offsets, counts, the reduction op, "all members enter a collective, or none") runs with more than one
// rank on a CPU, under the sanitizers (tests/sanitize/Makefile).  Built as a shared object with the soname librccl.so.1 and
// LINKED into the test programs, so that it is in the process when the group asks with RTLD_NOLOAD.  "Device memory" is host
// memory (fakehip/), the work is done on the calling threads, ranks are the members' threads.  Strict about what NCCL documents:
// see fakerccl.cc.  Not an RCCL implementation; never installed, never shipped.
//
// The entries are declared with the argument lists gamma_hip_group_rccl.h casts to (int for RCCL's enums, void* for
// ncclComm_t); fakerccl.cc static_asserts them equal, and tests/test_rccl_abi.py holds that header to the installed rccl.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

extern "C" {
int ncclCommInitAll(void** comm, int ndev, const int* devlist);
int ncclCommDestroy(void* comm);
int ncclAllGather(const void* sendbuff, void* recvbuff, size_t sendcount, int datatype, void* comm, hipStream_t stream);
int ncclAllReduce(const void* sendbuff, void* recvbuff, size_t count, int datatype, int op, void* comm, hipStream_t stream);
int ncclSend(const void* sendbuff, size_t count, int datatype, int peer, void* comm, hipStream_t stream);
int ncclRecv(void* recvbuff, size_t count, int datatype, int peer, void* comm, hipStream_t stream);
int ncclGroupStart();
int ncclGroupEnd();
const char* ncclGetErrorString(int result);

// ---- the stand-in's own entries (nothing the product reads) ----
struct fakerccl_counts { int64_t all_gather, all_reduce, send, recv, group_end; };   // calls made through ONE communicator
int fakerccl_get_counts(void* comm, fakerccl_counts* out);
void* fakerccl_live_comm(int nth);      // the nth communicator alive, in the order of creation (rank order of one ncclCommInitAll); or null
int fakerccl_comm_rank(void* comm);
int64_t fakerccl_comms_created(void);   // communicators ever created (ndev per successful ncclCommInitAll)
int64_t fakerccl_init_calls(void);      // calls of ncclCommInitAll, failed ones included
int64_t fakerccl_messages(void);        // "FAKE RCCL: ..." lines printed so far
void fakerccl_fail_next_init(int code); // the next ncclCommInitAll forms nothing and returns `code` (once)
}

// what rccl.h calls them
enum { fakeNcclSuccess = 0, fakeNcclInternalError = 3, fakeNcclInvalidArgument = 4, fakeNcclInvalidUsage = 5 };
enum { fakeNcclInt8 = 0, fakeNcclInt32 = 2, fakeNcclFloat32 = 7, fakeNcclFloat64 = 8, fakeNcclNumTypes = 10 };
enum { fakeNcclSum = 0, fakeNcclProd = 1, fakeNcclMax = 2, fakeNcclMin = 3 };
