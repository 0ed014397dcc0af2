// rccl_abi_check.cc -- TEST INFRASTRUCTURE, compiled with -fsyntax-only by tests/test_rccl_abi.py where <rccl/rccl.h> is
// installed: gamma_amd/csrc/gamma_hip_group_rccl.h writes RCCL's enumerators and the nine entries' pointer types out by hand
// (the group resolves the library by name at run time and is also built where the header does not exist).  Every one of them is
// held to the installed header here: the values, the sizes of the enums the group passes as int, and -- once ncclResult_t /
// ncclDataType_t / ncclRedOp_t are read as int and ncclComm_t as void* -- the exact type of every entry.  The stand-in
// communicator of the sanitizer programs (fakerccl/) static_asserts ITS declarations equal to the same struct.
#include <hip/hip_runtime_api.h>
#include <rccl/rccl.h>

#include <type_traits>

#include "../../gamma_amd/csrc/gamma_hip_group_rccl.h"

namespace {

using namespace gamma_group_rccl;

static_assert(kNcclChar == ncclInt8 && kNcclChar == ncclChar, "ncclInt8");
static_assert(kNcclFloat == ncclFloat32, "ncclFloat32");
static_assert(kNcclMax == ncclMax, "ncclMax");
static_assert(kNcclMin == ncclMin, "ncclMin");
static_assert(ncclSuccess == 0, "the group reads 0 as success");
static_assert(sizeof(ncclResult_t) == sizeof(int) && sizeof(ncclDataType_t) == sizeof(int) && sizeof(ncclRedOp_t) == sizeof(int),
              "the group passes and returns RCCL's enums as int");
static_assert(std::is_pointer<ncclComm_t>::value && sizeof(ncclComm_t) == sizeof(void*), "ncclComm_t: a pointer (void* in the group)");
static_assert(std::is_pointer<hipStream_t>::value, "hipStream_t: a pointer");

// the header's types as the group spells them
template <class T> struct Sub { typedef T type; };
template <> struct Sub<ncclResult_t> { typedef int type; };
template <> struct Sub<ncclDataType_t> { typedef int type; };
template <> struct Sub<ncclRedOp_t> { typedef int type; };
template <> struct Sub<ncclComm_t> { typedef void* type; };
template <> struct Sub<ncclComm_t*> { typedef void** type; };
template <class R, class... A> struct Sub<R (*)(A...)> { typedef typename Sub<R>::type (*type)(typename Sub<A>::type...); };

#define ENTRY(name, member)                                                                               \
    static_assert(std::is_same<Sub<decltype(&name)>::type, decltype(RcclApi::member)>::value,             \
                  #name ": RcclApi::" #member " is not its type with int for the enums and void* for ncclComm_t")
ENTRY(ncclCommInitAll, CommInitAll);
ENTRY(ncclCommDestroy, CommDestroy);
ENTRY(ncclAllGather, AllGather);
ENTRY(ncclAllReduce, AllReduce);
ENTRY(ncclSend, Send);
ENTRY(ncclRecv, Recv);
ENTRY(ncclGroupStart, GroupStart);
ENTRY(ncclGroupEnd, GroupEnd);
ENTRY(ncclGetErrorString, GetErrorString);

}  // namespace
