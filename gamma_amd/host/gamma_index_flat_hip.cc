// GammaFLATHIPIndex -- see gamma_index_flat_hip.h
#include "gamma_index_flat_hip.h"
#include "gamma_index_ivfpq_hip.h"   // WarnTiesNotHonoured

#include "filter_bridge.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <strings.h>

#include <algorithm>
#include <cmath>
#include <limits>

namespace tig_gamma {

REGISTER_MODEL(HIPFLAT, GammaFLATHIPIndex);

#define FLOG(...)                         \
  do {                                    \
    fprintf(stderr, "[HIPFLAT] ");        \
    fprintf(stderr, __VA_ARGS__);         \
    fprintf(stderr, "\n");                \
  } while (0)

namespace {
HIPFlatRowsFn &FlatRows() {
  static HIPFlatRowsFn fn = nullptr;
  return fn;
}
}  // namespace
int RegisterHIPFlatRows(HIPFlatRowsFn fn) {
  FlatRows() = fn;
  return 0;
}
HIPFlatRowsFn FindHIPFlatRows() { return FlatRows(); }

namespace {
HIPFlatSq8RowsFn &FlatSq8Rows() {
  static HIPFlatSq8RowsFn fn = nullptr;
  return fn;
}
}  // namespace
int RegisterHIPFlatSq8Rows(HIPFlatSq8RowsFn fn) {
  FlatSq8Rows() = fn;
  return 0;
}
HIPFlatSq8RowsFn FindHIPFlatSq8Rows() { return FlatSq8Rows(); }

int GammaFLATHIPIndex::ParseRawDtype(const std::string &model_parameters, int *et, float *sq8_range) {
  *et = 0;
  utils::JsonParser jp;
  std::string rdt;
  const bool parsed = model_parameters != "" && !jp.Parse(model_parameters.c_str());
  if (!(parsed && !jp.GetString("raw_dtype", rdt) && !strcasecmp("sq8", rdt.c_str()))) {
    // every other value: the answer shared with HIPIVFFLAT (gamma_index_ivfpq_hip.cc), which rejects "sq8"
    if (HIPParseRawDtype("HIPFLAT", model_parameters, et)) return -1;
    if (parsed && (jp.Contains("sq8_min") || jp.Contains("sq8_max"))) {
      FLOG("sq8_min / sq8_max come with \"raw_dtype\": \"sq8\" only");
      *et = 0;
      return -1;
    }
    return 0;
  }
  double lo = 0, hi = 0;
  if (jp.GetDouble("sq8_min", lo) || jp.GetDouble("sq8_max", hi)) {
    FLOG("raw_dtype = sq8 needs \"sq8_min\" and \"sq8_max\", one range for every dimension, as numbers");
    return -1;
  }
  const float flo = (float)lo, fhi = (float)hi;
  if (!std::isfinite(flo) || !std::isfinite(fhi) || !(flo <= fhi) || !std::isfinite(fhi - flo)) {
    FLOG("raw_dtype = sq8: sq8_min = %g, sq8_max = %g is no range (finite as floats, sq8_min <= sq8_max, a finite span)", lo, hi);
    return -1;
  }
  *et = 4;
  if (sq8_range) {
    sq8_range[0] = flo;
    sq8_range[1] = fhi;
  }
  return 0;
}

bool GammaFLATHIPIndex::RowsStorable(const char *what, const float *x, int64_t nrows) {
  if (raw_et_ == 4) {
    int64_t bad = -1;
    if (!raw_sq8_ops_->check(x, nrows * d_, &bad)) return true;
    FLOG("%s refused: raw_dtype = sq8 stores a value only if it is finite, and element %d of row %lld is %g", what, (int)(bad % d_),
         (long long)(bad / d_), (double)x[bad]);
    return false;
  }
  return raw_et_ < 2 || HIPRowsStorableI8(raw_i8_ops_, raw_et_ == 3, d_, "HIPFLAT", what, x, nrows);   // HIPIVFPQ's rule
}

GammaFLATHIPIndex::~GammaFLATHIPIndex() {
  if (h_) gamma_hip_destroy(h_);
}

int GammaFLATHIPIndex::Init(const std::string &model_parameters, int indexing_size) {
  indexing_size_ = indexing_size;
  if (!vector_) return -1;
  if (model_parameters != "") {   // FLATModelParams::Parse, gamma_index_flat.cc:34-55
    utils::JsonParser jp;
    if (jp.Parse(model_parameters.c_str())) return -1;
    std::string mt;
    if (!jp.GetString("metric_type", mt)) {
      if (strcasecmp("L2", mt.c_str()) && strcasecmp("InnerProduct", mt.c_str())) return -1;
      metric_type_ = !strcasecmp("L2", mt.c_str()) ? DistanceComputeType::L2 : DistanceComputeType::INNER_PRODUCT;
    }
    int v = 0;
    if (!jp.GetInt("device_filters", v)) device_filters_ = v != 0;   // HIP only, see filter_bridge.h
    if (!jp.GetInt("exact_ties", v)) exact_ties_ = v != 0;           // HIP only: the reference's heap order inside ties (default on)
  }
  float sq8_range[2] = {0.f, 0.f};
  if (ParseRawDtype(model_parameters, &raw_et_, sq8_range)) return -1;
  // a narrow store needs its initialiser and the handle's switch; a build without one of them rejects the value
  const bool narrow = raw_et_ >= 1 && raw_et_ <= 3;
  const HIPFlatRowsFn flat_rows = narrow ? FindHIPFlatRows() : nullptr;
  const HIPRawInitFn init_f16 = raw_et_ == 1 ? FindHIPRawInitF16() : nullptr;
  raw_i8_ops_ = raw_et_ == 2 || raw_et_ == 3 ? FindHIPRawI8() : nullptr;
  if (narrow && (!flat_rows || (raw_et_ == 1 ? !init_f16 : !raw_i8_ops_))) {
    FLOG("raw_dtype: this build of the plugin has no flat search over float16 / uint8 / int8 rows");
    return -1;
  }
  // (sq8: the store's entries that HIPIVFPQ's sq8 store registered, and a switch of its own)
  const HIPFlatSq8RowsFn flat_sq8_rows = raw_et_ == 4 ? FindHIPFlatSq8Rows() : nullptr;
  raw_sq8_ops_ = raw_et_ == 4 ? FindHIPRawSq8() : nullptr;
  if (raw_et_ == 4 && (!flat_sq8_rows || !raw_sq8_ops_)) {
    FLOG("raw_dtype: this build of the plugin has no flat search over sq8 rows");
    return -1;
  }
  d_ = vector_->MetaInfo()->Dimension();
  const char *dev = getenv("GAMMA_HIP_DEVICE");
  if (gamma_hip_create(dev ? atoi(dev) : 0, &h_)) return -1;
  if (gamma_hip_set_exact_ties(h_, exact_ties_ ? 1 : 0)) return -1;
  if (!raw_et_) return gamma_hip_raw_init(h_, d_) ? -1 : 0;
  if (raw_et_ == 4) {   // one range for every dimension, from the parameters (Load re-encodes with the same)
    const std::vector<float> vmin((size_t)d_, sq8_range[0]), vmax((size_t)d_, sq8_range[1]);
    if (raw_sq8_ops_->init(h_, d_) || raw_sq8_ops_->set_ranges(h_, vmin.data(), vmax.data())) return -1;
    return flat_sq8_rows(h_, 1) ? -1 : 0;
  }
  if (raw_et_ == 1 ? init_f16(h_, d_) : raw_i8_ops_->init(h_, d_, raw_et_ == 3)) return -1;
  return flat_rows(h_, 1) ? -1 : 0;
}

RetrievalParameters *GammaFLATHIPIndex::Parse(const std::string &parameters) {
  if (parameters == "") return new HIPFlatRetrievalParameters(metric_type_);
  utils::JsonParser jp;
  if (jp.Parse(parameters.c_str())) return nullptr;
  DistanceComputeType type = metric_type_;
  std::string mt;
  if (!jp.GetString("metric_type", mt))
    type = !strcasecmp("L2", mt.c_str()) ? DistanceComputeType::L2 : DistanceComputeType::INNER_PRODUCT;
  int poq = 1;
  jp.GetInt("parallel_on_queries", poq);
  HIPFlatRetrievalParameters *rp = new HIPFlatRetrievalParameters(poq != 0, type);
  int et = 0;
  if (!jp.GetInt("exact_ties", et)) rp->SetExactTies(et != 0 ? 1 : -1);
  return rp;
}

bool GammaFLATHIPIndex::Add(int n, const uint8_t *vec) {
  // the CPU model reads vector_ at search time; the device keeps a mirror, fed in vid order at explicit rows
  if (!RowsStorable("add", reinterpret_cast<const float *>(vec), n)) return false;   // before anything changes
  std::lock_guard<std::mutex> g(raw_mu_);
  if (gamma_hip_raw_write(h_, uploaded_, n, reinterpret_cast<const float *>(vec))) return false;
  uploaded_ += n;
  return SyncVid2DocID(uploaded_) == 0;
}

// multi-vector documents: docids of the mirrored vids to the device (filters and the delete bitmap are on DOC ids)
int GammaFLATHIPIndex::SyncVid2DocID(int64_t upto) {
  RawVector *rv = dynamic_cast<RawVector *>(vector_);
  if (!rv || !rv->VidMgr() || !rv->VidMgr()->MultiVids()) return 0;
  const int64_t have = gamma_hip_vid2docid_count(h_);
  if (have < 0) return -1;
  if (upto <= have) return 0;
  std::vector<int32_t> m((size_t)(upto - have));
  for (int64_t v = have; v < upto; v++) m[(size_t)(v - have)] = rv->VidMgr()->VID2DocID((int)v);
  return gamma_hip_vid2docid_append(h_, (int64_t)m.size(), m.data());
}

int GammaFLATHIPIndex::Update(const std::vector<int64_t> &ids, const std::vector<const uint8_t *> &vecs) {
  for (size_t i = 0; i < ids.size(); i++)   // every row before any is written
    if (!RowsStorable("update", reinterpret_cast<const float *>(vecs[i]), 1)) return -1;
  std::lock_guard<std::mutex> g(raw_mu_);
  for (size_t i = 0; i < ids.size(); i++)
    if (ids[i] < uploaded_ && gamma_hip_raw_update(h_, ids[i], reinterpret_cast<const float *>(vecs[i]))) return -1;
  return 0;
}

int GammaFLATHIPIndex::Delete(const std::vector<int64_t> &ids) {
  if (ids.empty()) return 0;
  std::vector<int64_t> docs(ids);   // the bitmap is on DOC ids (VIDMgr::VID2DocID; identity for single-vector documents)
  RawVector *rv = dynamic_cast<RawVector *>(vector_);
  if (rv && rv->VidMgr() && rv->VidMgr()->MultiVids())
    for (size_t i = 0; i < docs.size(); i++) docs[i] = rv->VidMgr()->VID2DocID((int)ids[i]);
  return gamma_hip_bitmap_set(h_, docs.data(), (int64_t)docs.size(), 1) ? -1 : 0;
}

int GammaFLATHIPIndex::Load(const std::string &dir) {
  // deletes made before the restart: the engine has loaded its bitmap file already (vector_ is a RawVector)
  if (RawVector *rv = dynamic_cast<RawVector *>(vector_)) {
    if (rv->Bitmap() && rv->Bitmap()->BitSize() > 0 &&
        gamma_hip_bitmap_upload(h_, reinterpret_cast<const uint8_t *>(rv->Bitmap()->Bitmap()),
                                (int64_t)rv->Bitmap()->BitSize()))
      return -1;
  }
  std::lock_guard<std::mutex> g(raw_mu_);
  const int64_t nvec = (int64_t)vector_->MetaInfo()->Size();
  // a byte or sq8 model: a pass over the rows with the acceptance predicate first, so that a refused row leaves the mirror as it was
  for (int pass = raw_et_ >= 2 ? 0 : 1; pass < 2; pass++)
    for (int64_t i0 = uploaded_; i0 < nvec; i0 += 65536) {
      const int64_t nb = std::min<int64_t>(65536, nvec - i0);
      std::vector<int64_t> vids(nb);
      for (int64_t i = 0; i < nb; i++) vids[i] = i0 + i;
      ScopeVectors sv;
      if (vector_->Gets(vids, sv)) return -1;
      std::vector<float> buf((size_t)nb * d_);
      for (int64_t i = 0; i < nb; i++) memcpy(&buf[(size_t)i * d_], sv.Get((int)i), sizeof(float) * d_);
      if (pass == 0) {
        if (!RowsStorable("load", buf.data(), nb)) return -1;
        continue;
      }
      if (gamma_hip_raw_write(h_, i0, nb, buf.data())) return -1;
      uploaded_ = i0 + nb;
    }
  if (SyncVid2DocID(uploaded_)) return -1;
  return (int)uploaded_;
}

int GammaFLATHIPIndex::Search(RetrievalContext *retrieval_context, int n, const uint8_t *x, int k,
                              float *distances, int64_t *ids) {
  HIPFlatRetrievalParameters *rp = dynamic_cast<HIPFlatRetrievalParameters *>(retrieval_context->RetrievalParams());
  HIPFlatRetrievalParameters defaults(true, DistanceComputeType::L2);   // gamma_index_flat.cc:125-128
  if (rp == nullptr) rp = &defaults;
  if (x == nullptr) return -1;
  GammaSearchCondition *cond = dynamic_cast<GammaSearchCondition *>(retrieval_context);
  gamma_hip_search_params p;
  memset(&p, 0, sizeof(p));
  p.metric = rp->GetDistanceComputeType() == DistanceComputeType::INNER_PRODUCT ? GAMMA_HIP_METRIC_IP
                                                                                : GAMMA_HIP_METRIC_L2;
  p.min_score = cond ? cond->min_score : std::numeric_limits<float>::min();
  p.max_score = cond ? cond->max_score : std::numeric_limits<float>::max();
  p.exact_ties = rp->ExactTies();
  std::vector<gamma_hip_range_filter> rf;
  std::vector<gamma_hip_field_filter> ff;
  std::vector<gamma_hip_term_filter> tf;
  if (!(device_filters_ && columns_.Prepare(h_, cond, DocCountOf(this, (int64_t)vector_->MetaInfo()->Size()), p, ff, tf)))
    FillRangeFilters(cond, p, rf);
  const int rc = gamma_hip_flat_search(h_, &p, n, reinterpret_cast<const float *>(x), k, distances, ids);
  if (!rc) WarnTiesNotHonoured(h_, nullptr, &ties_said_);
  return rc;
}

}  // namespace tig_gamma
