// GammaBinaryIVFHIPIndex -- see gamma_index_binivf_hip.h
#include "gamma_index_binivf_hip.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <limits>

namespace tig_gamma {

REGISTER_MODEL(HIPBINARYIVF, GammaBinaryIVFHIPIndex);

#define BLOG(...)                                  \
  do {                                             \
    fprintf(stderr, "[HIPBINARYIVF] " __VA_ARGS__); \
    fprintf(stderr, "\n");                         \
  } while (0)

GammaBinaryIVFHIPIndex::~GammaBinaryIVFHIPIndex() {
  if (h_) gamma_hip_destroy(h_);
}

// Init (gamma_index_binary_ivf.cc:82-124): BinaryModelParams hold ncentroids only (default 256); the model's nprobe is 20
// whatever the parameters say; d = Dimension() * 8 bits; bucket_keys = max(1000, indexing_size / ncentroids), at most
// 1280000 entries per list
int GammaBinaryIVFHIPIndex::Init(const std::string &model_parameters, int indexing_size) {
  indexing_size_ = indexing_size;
  if (!vector_) return -1;
  if (model_parameters != "") {
    utils::JsonParser jp;
    if (jp.Parse(model_parameters.c_str())) return -1;
    int v = 0;
    if (!jp.GetInt("ncentroids", v)) {   // BinaryModelParams::Parse (:16-55): a value <= 0 other than -1 is an error
      if (v > 0) nlist_ = v;
      else if (v != -1) return -1;
    }
    if (!jp.GetInt("device_filters", v)) device_filters_ = v != 0;   // HIP only, see filter_bridge.h
  }
  nprobe_ = 20;
  nbits_ = vector_->MetaInfo()->Dimension() * 8;
  const int bucket_keys = std::max(1000, indexing_size_ / nlist_);
  const char *dev = getenv("GAMMA_HIP_DEVICE");
  if (gamma_hip_create(dev ? atoi(dev) : 0, &h_)) return -1;
  const int rc = gamma_hip_binivf_init(h_, nbits_, nlist_, bucket_keys, 1280000);
  if (rc) {
    BLOG("device init failed: %s (%s)", gamma_hip_strerror(rc), gamma_hip_last_error(h_));
    return -1;
  }
  return 0;
}

// Parse (:126-146): the JSON nprobe when it is > 0
RetrievalParameters *GammaBinaryIVFHIPIndex::Parse(const std::string &parameters) {
  if (parameters == "") return new HIPBinaryIVFRetrievalParameters();
  utils::JsonParser jp;
  if (jp.Parse(parameters.c_str())) {
    BLOG("parse retrieval parameters error: %s", parameters.c_str());
    return nullptr;
  }
  HIPBinaryIVFRetrievalParameters *rp = new HIPBinaryIVFRetrievalParameters();
  int nprobe = 0;
  if (!jp.GetInt("nprobe", nprobe) && nprobe > 0) rp->SetNprobe(nprobe);
  return rp;
}

// Indexing (:208-266): the first `num` vectors of the store, num = nlist * 39 when indexing_size < nlist, else
// indexing_size capped at nlist * 256; fewer vectors in the store than that: -1
int GammaBinaryIVFHIPIndex::Indexing() {
  if (is_trained_) return 0;
  const size_t count = vector_->MetaInfo()->Size();
  size_t num;
  if ((size_t)indexing_size_ < (size_t)nlist_) num = (size_t)nlist_ * 39;
  else if ((size_t)indexing_size_ <= (size_t)nlist_ * 256) num = (size_t)indexing_size_;
  else num = (size_t)nlist_ * 256;
  if (num > count) {
    BLOG("vector total count [%zu] less then index_size[%zu], failed!", count, num);
    return -1;
  }
  const int cs = nbits_ / 8;
  std::vector<uint8_t> codes(num * cs);
  for (size_t i0 = 0; i0 < num; i0 += 65536) {
    const size_t nb = std::min<size_t>(65536, num - i0);
    std::vector<int64_t> vids(nb);
    for (size_t i = 0; i < nb; i++) vids[i] = (int64_t)(i0 + i);
    ScopeVectors sv;
    if (vector_->Gets(vids, sv)) return -1;
    for (size_t i = 0; i < nb; i++) memcpy(&codes[(i0 + i) * cs], sv.Get((int)i), cs);
  }
  std::vector<uint8_t> cc((size_t)nlist_ * cs);
  int rc = gamma_hip_binivf_train(h_, nbits_, (int64_t)num, codes.data(), nlist_, cc.data());
  if (!rc) rc = gamma_hip_binivf_set_trained(h_, cc.data());
  if (rc) {
    BLOG("training failed: %s (%s)", gamma_hip_strerror(rc), gamma_hip_last_error(h_));
    return -1;
  }
  is_trained_ = true;
  return 0;
}

// multi-vector documents: docids of the indexed vids to the device (the filters and the delete bitmap are on DOC ids)
int GammaBinaryIVFHIPIndex::SyncVid2DocID(int64_t upto) {
  RawVector *rv = dynamic_cast<RawVector *>(vector_);
  if (!rv || !rv->VidMgr() || !rv->VidMgr()->MultiVids()) return 0;
  const int64_t have = gamma_hip_vid2docid_count(h_);
  if (have < 0) return -1;
  if (upto <= have) return 0;
  std::vector<int32_t> m((size_t)(upto - have));
  for (int64_t v = have; v < upto; v++) m[(size_t)(v - have)] = rv->VidMgr()->VID2DocID((int)v);
  return gamma_hip_vid2docid_append(h_, (int64_t)m.size(), m.data());
}

// mirror rows [flat_mirrored_, upto) of the engine's store into the flat store of the exact search, and their docids.
// Called from Search (any number of client threads); add_mu_ makes "read the watermark, copy, advance it" one step and
// keeps it apart from Add's vid -> docid sync.  Update is the reference's no-op, so a mirrored row never changes.
int GammaBinaryIVFHIPIndex::EnsureFlat(int64_t upto) {
  std::lock_guard<std::mutex> g(add_mu_);
  int rc = 0;
  if (!flat_init_) {
    if ((rc = gamma_hip_binflat_init(h_, nbits_))) {
      BLOG("flat store init failed: %s (%s)", gamma_hip_strerror(rc), gamma_hip_last_error(h_));
      return -1;
    }
    flat_init_ = true;
  }
  const int cs = nbits_ / 8;
  const int64_t step = 65536;
  for (int64_t i0 = flat_mirrored_; i0 < upto; i0 += step) {
    const int64_t nb = std::min(step, upto - i0);
    std::vector<int64_t> vids((size_t)nb);
    for (int64_t i = 0; i < nb; i++) vids[(size_t)i] = i0 + i;
    ScopeVectors sv;
    if (vector_->Gets(vids, sv)) return -1;
    std::vector<uint8_t> buf((size_t)nb * cs);
    for (int64_t i = 0; i < nb; i++) memcpy(&buf[(size_t)i * cs], sv.Get((int)i), cs);
    if ((rc = gamma_hip_binflat_append(h_, nb, buf.data()))) {
      BLOG("flat store append failed: %s (%s)", gamma_hip_strerror(rc), gamma_hip_last_error(h_));
      return -1;
    }
    flat_mirrored_ = i0 + nb;
  }
  return SyncVid2DocID(flat_mirrored_) ? -1 : 0;
}

// Add (:148-206): assign + AddKeys, vids from indexed_vec_count_; before training the reference throws -- false here
bool GammaBinaryIVFHIPIndex::Add(int n, const uint8_t *vec) {
  if (!is_trained_) return false;
  std::lock_guard<std::mutex> g(add_mu_);
  if (SyncVid2DocID(indexed_vec_count_ + n)) return false;
  const int rc = gamma_hip_binivf_add(h_, n, vec, indexed_vec_count_);
  if (rc) {
    BLOG("add failed: %s (%s)", gamma_hip_strerror(rc), gamma_hip_last_error(h_));
    return false;
  }
  indexed_vec_count_ += n;
  return true;
}

// Delete (:275-279): RTInvertIndex::Delete only counts; the engine's bitmap (mirrored on the device) decides validity
int GammaBinaryIVFHIPIndex::Delete(const std::vector<int64_t> &ids) {
  if (ids.empty()) return 0;
  std::vector<int64_t> docs(ids);
  RawVector *rv = dynamic_cast<RawVector *>(vector_);
  if (rv && rv->VidMgr() && rv->VidMgr()->MultiVids())
    for (size_t i = 0; i < docs.size(); i++) docs[i] = rv->VidMgr()->VID2DocID((int)ids[i]);
  if (gamma_hip_bitmap_set(h_, docs.data(), (int64_t)docs.size(), 1)) return -1;
  return gamma_hip_ivfpq_delete(h_, ids.data(), (int)ids.size()) ? -1 : 0;
}

// Search (:281-404): the request's nprobe if it lies in (0, nlist], else 20 (the C ABI applies the rule); the score
// window of the search condition; distances are Hamming distances as floats, empty slots (float)INT32_MAX / -1
int GammaBinaryIVFHIPIndex::Search(RetrievalContext *retrieval_context, int n, const uint8_t *x, int k, float *distances,
                                   int64_t *ids) {
  if (x == nullptr) return -1;
  HIPBinaryIVFRetrievalParameters *rp =
      dynamic_cast<HIPBinaryIVFRetrievalParameters *>(retrieval_context->RetrievalParams());
  HIPBinaryIVFRetrievalParameters defaults;
  if (rp == nullptr) rp = &defaults;
  GammaSearchCondition *cond = dynamic_cast<GammaSearchCondition *>(retrieval_context);
  // brute_force_search, and every search of a model that is not trained yet, is the exact Hamming search over all the rows
  // the engine's store holds (the float models send both to their flat search)
  const bool brute = (cond && cond->brute_force_search) || !is_trained_;
  if (brute && EnsureFlat((int64_t)vector_->MetaInfo()->Size())) return -1;
  gamma_hip_search_params p;
  memset(&p, 0, sizeof(p));
  p.metric = GAMMA_HIP_METRIC_L2;
  p.nprobe = (rp->Nprobe() > 0 && rp->Nprobe() <= nlist_) ? rp->Nprobe() : nprobe_;
  p.min_score = cond ? cond->min_score : std::numeric_limits<float>::min();
  p.max_score = cond ? cond->max_score : std::numeric_limits<float>::max();
  std::vector<gamma_hip_range_filter> rf;
  std::vector<gamma_hip_field_filter> ff;
  std::vector<gamma_hip_term_filter> tf;
  if (!(device_filters_ && columns_.Prepare(h_, cond, DocCountOf(this, (int64_t)vector_->MetaInfo()->Size()), p, ff, tf)))
    FillRangeFilters(cond, p, rf);
  const int rc = brute ? gamma_hip_binflat_search(h_, &p, n, x, k, distances, ids)
                       : gamma_hip_binivf_search(h_, &p, n, x, k, distances, ids);
  if (rc) BLOG("%ssearch failed: %s (%s)", brute ? "brute-force " : "", gamma_hip_strerror(rc), gamma_hip_last_error(h_));
  return rc;
}

}  // namespace tig_gamma
