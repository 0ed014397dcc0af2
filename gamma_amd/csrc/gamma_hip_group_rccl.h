// gamma_hip_group_rccl.h -- the part of RCCL's ABI that gamma_hip_group.cpp resolves at run time by name (dlopen / dlsym: no
// link-time dependency on the library): the nine entries as function pointers, and the enumerators it passes.  Written out
// here, not taken from <rccl/rccl.h>, because the group is also built where that header does not exist; tests/test_rccl_abi.py
// compiles this file beside the installed header and static_asserts every value and every pointer type below against it
// (ncclResult_t / ncclDataType_t / ncclRedOp_t: int; ncclComm_t: void*).
//
// Include the HIP runtime header first: hipStream_t is its.
#pragma once
#include <stddef.h>

namespace gamma_group_rccl {

struct RcclApi {
    void* lib = nullptr;
    int (*CommInitAll)(void**, int, const int*) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*Send)(const void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*Recv)(void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    bool ok() const { return CommInitAll && CommDestroy && AllGather && AllReduce && Send && Recv && GroupStart && GroupEnd; }
};
constexpr int kNcclChar = 0;   // ncclInt8: the exchanges are counted in bytes
constexpr int kNcclFloat = 7, kNcclMax = 2, kNcclMin = 3;   // ncclFloat32, ncclMax, ncclMin (nccl.h)

}  // namespace gamma_group_rccl
