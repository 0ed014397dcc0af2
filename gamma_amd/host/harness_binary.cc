// harness_binary.cc -- extern "C" test harness for the binary models (HIPBINARYIVF), driven the way VectorManager drives a
// model over a BINARY raw vector store (vector/vector_manager.cc:161-192): create by name through the reflector, set
// vector_, Init, store, Indexing, Add, Parse + Search with a GammaSearchCondition.  Rows are codes of Dimension() bytes.
// Used by the Python tests through ctypes (gamma_amd/plugin.py, BinaryPluginModel); not part of the product surface.
#include <string.h>

#include <mutex>
#include <string>
#include <vector>

#include "gamma_index_binivf_hip.h"
#include "plugin_api.h"

using namespace tig_gamma;

namespace {
// MemoryRawVector stand-in with VectorValueType::BINARY: dimension in bytes, the engine's delete bitmap behind Bitmap()
class MemBinaryVectorReader : public RawVector {
 public:
  explicit MemBinaryVectorReader(int d_bytes)
      : RawVector(new VectorMetaInfo("vec", d_bytes, VectorValueType::BINARY), &bitmap_), d_(d_bytes) {
    bitmap_.Init(1 << 22);
  }
  int Gets(const std::vector<int64_t> &vids, ScopeVectors &vecs) const override {
    std::lock_guard<std::mutex> g(mu_);
    for (auto v : vids) {
      if (v < 0 || (size_t)v >= data_.size() / d_) return -1;
      uint8_t *c = new uint8_t[d_];
      memcpy(c, &data_[(size_t)v * d_], d_);
      vecs.Add(c, true);
    }
    return 0;
  }
  void Append(int n, const uint8_t *x) {
    std::lock_guard<std::mutex> g(mu_);
    data_.insert(data_.end(), x, x + (size_t)n * d_);
    meta_info_->size_ += n;
  }
  int d_;
  std::vector<uint8_t> data_;
  bitmap::BitmapManager bitmap_;
  mutable std::mutex mu_;
};

struct BinHost {
  MemBinaryVectorReader *store;
  RetrievalModel *model;
};
}  // namespace

extern "C" {

void *gh_bin_new(const char *retrieval_type, int d_bytes) {
  RetrievalModel *m = reflector().GetNewModel(retrieval_type);
  if (!m) return nullptr;
  BinHost *h = new BinHost();
  h->store = new MemBinaryVectorReader(d_bytes);
  h->model = m;
  m->vector_ = h->store;
  return h;
}
void gh_bin_free(void *hp) {
  BinHost *h = (BinHost *)hp;
  delete h->model;
  delete h->store;
  delete h;
}
int gh_bin_init(void *hp, const char *model_param, int indexing_size) {
  return ((BinHost *)hp)->model->Init(model_param, indexing_size);
}
// AddToStore without indexing
void gh_bin_store(void *hp, int n, const uint8_t *x) { ((BinHost *)hp)->store->Append(n, x); }
int gh_bin_indexing(void *hp) { return ((BinHost *)hp)->model->Indexing(); }
// model->Add for codes already in the store; 1 = added
int gh_bin_add(void *hp, int n, const uint8_t *x) {
  BinHost *h = (BinHost *)hp;
  const bool ok = h->model->Add(n, x);
  if (ok) h->model->indexed_count_ += n;
  return ok ? 1 : 0;
}
int gh_bin_update(void *hp, int64_t vid, const uint8_t *x) {
  BinHost *h = (BinHost *)hp;
  std::vector<int64_t> ids{vid};
  std::vector<const uint8_t *> vecs{x};
  return h->model->Update(ids, vecs);
}
// GammaEngine::Delete: the doc bit in the engine's bitmap, then the model
int gh_bin_delete(void *hp, const int64_t *vids, int n) {
  BinHost *h = (BinHost *)hp;
  for (int i = 0; i < n; i++) h->store->bitmap_.Set((uint32_t)vids[i]);
  std::vector<int64_t> ids(vids, vids + n);
  return h->model->Delete(ids);
}
// Search with the condition's score window and n_range range results (docids of range i: counts[i] entries)
int gh_bin_search(void *hp, const char *retrieval_params, float min_score, float max_score, int n, const uint8_t *x, int k,
                  float *distances, int64_t *ids, int n_range, const int64_t *docids, const int *counts, const int *not_in) {
  BinHost *h = (BinHost *)hp;
  PerfTool perf;
  GammaSearchCondition cond(&perf);
  MultiRangeQueryResults mr;
  size_t off = 0;
  for (int i = 0; i < n_range; i++) {
    RangeQueryResult r;
    if (counts[i] > 0) {
      for (int j = 0; j < counts[i]; j++) r.SetRange((int)docids[off + j], (int)docids[off + j]);
    } else {
      r.SetRange(0, 0);
    }
    r.Resize();
    for (int j = 0; j < counts[i]; j++) r.Set((int)docids[off + j] - r.MinAligned());
    r.SetNotIn(not_in[i] != 0);
    off += counts[i];
    mr.Add(std::move(r));
  }
  if (n_range > 0) cond.range_query_result = &mr;
  cond.topn = k;
  cond.min_score = min_score;
  cond.max_score = max_score;
  cond.retrieval_params_ = h->model->Parse(retrieval_params);
  if (!cond.retrieval_params_) return -100;
  return h->model->Search(&cond, n, x, k, distances, ids);
}
// gh_bin_search with GammaSearchCondition::brute_force_search = (brute != 0)
int gh_bin_search_brute(void *hp, const char *retrieval_params, float min_score, float max_score, int n, const uint8_t *x,
                        int k, float *distances, int64_t *ids, int n_range, const int64_t *docids, const int *counts,
                        const int *not_in, int brute) {
  BinHost *h = (BinHost *)hp;
  PerfTool perf;
  GammaSearchCondition cond(&perf);
  MultiRangeQueryResults mr;
  size_t off = 0;
  for (int i = 0; i < n_range; i++) {
    RangeQueryResult r;
    if (counts[i] > 0) {
      for (int j = 0; j < counts[i]; j++) r.SetRange((int)docids[off + j], (int)docids[off + j]);
    } else {
      r.SetRange(0, 0);
    }
    r.Resize();
    for (int j = 0; j < counts[i]; j++) r.Set((int)docids[off + j] - r.MinAligned());
    r.SetNotIn(not_in[i] != 0);
    off += counts[i];
    mr.Add(std::move(r));
  }
  if (n_range > 0) cond.range_query_result = &mr;
  cond.topn = k;
  cond.min_score = min_score;
  cond.max_score = max_score;
  cond.brute_force_search = brute != 0;
  cond.retrieval_params_ = h->model->Parse(retrieval_params);
  if (!cond.retrieval_params_) return -100;
  return h->model->Search(&cond, n, x, k, distances, ids);
}
int gh_bin_dump(void *hp, const char *dir) { return ((BinHost *)hp)->model->Dump(dir); }
int gh_bin_load(void *hp, const char *dir) { return ((BinHost *)hp)->model->Load(dir); }
long gh_bin_mem_bytes(void *hp) { return ((BinHost *)hp)->model->GetTotalMemBytes(); }
// the model's state after Init / Indexing: nlist, nprobe, nbits, trained
void gh_bin_binivf_state(void *hp, int *out4) {
  GammaBinaryIVFHIPIndex *m = dynamic_cast<GammaBinaryIVFHIPIndex *>(((BinHost *)hp)->model);
  out4[0] = m ? m->nlist_ : -1;
  out4[1] = m ? m->nprobe_ : -1;
  out4[2] = m ? m->nbits_ : -1;
  out4[3] = m ? (int)m->is_trained_ : -1;
}

}  // extern "C"
