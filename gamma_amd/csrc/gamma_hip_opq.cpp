// gamma_hip_opq.cpp -- the OPQ rotation on a handle (include/gamma_hip.h, gamma_hip_opq_*): the matrix the reference keeps as
// faiss::OPQMatrix* opq_ (index/impl/gamma_index_ivfpq.h:745, gamma_index_ivfpq.cc:155-166) and applies in front of the coarse
// quantizer and the PQ encoder (Add :424-512, Update :375-422) and in front of the search (:514-566).  Setting it is all a
// caller does: the entry points that quantise vectors rotate them inside the library (gamma_hip_store.cpp encode_host,
// gamma_hip_search.cpp ivfpq_search_device_locked); the arithmetic is opq.hip's.
#include "gamma_hip_group_ext.h"
#include "gamma_hip_internal.h"
#include "opq.h"
#include "pq4.h"

using namespace ghi;

extern "C" {

int gamma_hip_opq_set(gamma_hip_index* h, const float* A) {
    if (!h) return GAMMA_HIP_EINVAL;
    WriteLock lk(h);
    if (!h->ivf_init) return fail(h, GAMMA_HIP_EINVAL, "opq_set: ivfpq not initialised");
    if (h->binivf) return fail(h, GAMMA_HIP_EUNSUPPORTED, "opq_set: a binary IVF handle has no rotation");
    if (h->ivfflat) return fail(h, GAMMA_HIP_EUNSUPPORTED, "opq_set: an IVFFLAT handle has no rotation");
    if (h->ksub == gh::kPq4Ksub) return fail(h, GAMMA_HIP_EUNSUPPORTED, "opq_set: OPQ with 4-bit codes is not supported");
    if (h->group_member) return fail(h, GAMMA_HIP_EUNSUPPORTED, "opq_set: OPQ on a member of a group is not supported");
    if (!h->h_list_mask.empty()) return fail(h, GAMMA_HIP_EUNSUPPORTED, "opq_set: OPQ on a list shard is not supported");
    if (!A) return fail(h, GAMMA_HIP_EINVAL, "opq_set: null matrix");
    bool any = h->ntotal > 0;
    for (int l : h->h_list_len) any |= l > 0;
    if (any)
        return fail(h, GAMMA_HIP_EINVAL, "opq_set: the lists already hold entries (their codes are of unrotated vectors)");
    GH_CHECK(h, hipSetDevice(h->device));
    GH_CHECK(h, lk.exclusive());   // a search of the empty index may be reading the matrix this call replaces
    const size_t bytes = (size_t)h->d * h->d * sizeof(float);
    if (!h->d_opq) GH_CHECK(h, hipMalloc((void**)&h->d_opq, bytes));
    h->h_opq.assign(A, A + (size_t)h->d * h->d);
    GH_CHECK(h, hipMemcpyAsync(h->d_opq, h->h_opq.data(), bytes, hipMemcpyHostToDevice, h->wstream));
    GH_CHECK(h, hipStreamSynchronize(h->wstream));
    return GAMMA_HIP_OK;
}

int gamma_hip_opq_get(gamma_hip_index* h, float* A_out) {
    if (!h) return GAMMA_HIP_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    if (!h->d_opq) return 0;
    if (A_out) memcpy(A_out, h->h_opq.data(), h->h_opq.size() * sizeof(float));
    return 1;
}

int gamma_hip_opq_apply(gamma_hip_index* h, int64_t n, const float* x, float* xt) {
    if (!h || n < 0 || (n > 0 && (!x || !xt))) return GAMMA_HIP_EINVAL;
    WriteLock lk(h);   // the writers' stream and workspaces: runs beside the searches
    if (!h->d_opq) return fail(h, GAMMA_HIP_EINVAL, "opq_apply: no OPQ matrix set");
    if (n == 0) return GAMMA_HIP_OK;
    GH_CHECK(h, hipSetDevice(h->device));
    const int d = h->d;
    const int64_t chunk = std::min<int64_t>(n, 65536);
    GH_CHECK(h, h->we_x.ensure((size_t)chunk * d * sizeof(float)));
    GH_CHECK(h, h->we_xrot.ensure((size_t)chunk * d * sizeof(float)));
    for (int64_t i0 = 0; i0 < n; i0 += chunk) {
        const int64_t nc = std::min(chunk, n - i0);
        GH_CHECK(h, hipMemcpyAsync(h->we_x.p, x + i0 * d, (size_t)nc * d * sizeof(float), hipMemcpyHostToDevice, h->wstream));
        gh::launch_opq_apply(h->wstream, h->d_opq, d, h->we_x.as<float>(), nc, h->we_xrot.as<float>());
        GH_CHECK(h, hipGetLastError());
        GH_CHECK(h, hipMemcpyAsync(xt + i0 * d, h->we_xrot.p, (size_t)nc * d * sizeof(float), hipMemcpyDeviceToHost, h->wstream));
        GH_CHECK(h, hipStreamSynchronize(h->wstream));
    }
    return GAMMA_HIP_OK;
}

int gamma_hip_opq_apply_device(gamma_hip_index* h, int64_t n, const float* d_x, float* d_xt) {
    if (!h || n < 0 || (n > 0 && (!d_x || !d_xt))) return GAMMA_HIP_EINVAL;
    SearchLock lk(h);
    if (!h->d_opq) return fail(h, GAMMA_HIP_EINVAL, "opq_apply_device: no OPQ matrix set");
    if (n == 0) return GAMMA_HIP_OK;
    if (d_x == d_xt) return fail(h, GAMMA_HIP_EINVAL, "opq_apply_device: in place is not supported");
    GH_CHECK(h, hipSetDevice(h->device));
    gh::launch_opq_apply(h->stream, h->d_opq, h->d, d_x, n, d_xt);
    GH_CHECK(h, hipGetLastError());
    return GAMMA_HIP_OK;
}

}  // extern "C"

// gamma_hip_group_ext.h: the group marks its members through this function, registered here -- beside gamma_hip_opq_set, the
// one entry the mark matters to
namespace {
int mark_group_member(gamma_hip_index* h) {
    if (!h) return GAMMA_HIP_EINVAL;
    std::lock_guard<std::mutex> g(h->mu);
    h->group_member = true;
    return GAMMA_HIP_OK;
}
const int member_mark_registered = gamma_group_ext::register_member_mark(mark_group_member);
}  // namespace
