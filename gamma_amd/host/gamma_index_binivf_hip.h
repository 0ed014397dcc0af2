// GammaBinaryIVFHIPIndex -- RetrievalModel plugin "HIPBINARYIVF": Gamma's binary IVF model
// (reference index/impl/gamma_index_binary_ivf.{h,cc}) on an MI355X.  Same JSON keys ("ncentroids" in the model
// parameters, "nprobe" in the retrieval parameters), same Init / Indexing / Add / Search contract; Update, Dump and Load
// are the reference's no-ops (gamma_index_binary_ivf.h:99-104).  The store is a BINARY RawVector whose Dimension() counts
// bytes.  HIP only: brute_force_search, and the search of a model that is not trained yet, answer exactly over every row
// of the store (gamma_hip_binflat_search over a mirror kept by EnsureFlat; the reference returns -1 / ignores the flag).
#pragma once
#include <atomic>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/gamma_hip.h"
#include "filter_bridge.h"
#include "plugin_includes.h"

namespace tig_gamma {

class HIPBinaryIVFRetrievalParameters : public RetrievalParameters {
 public:
  HIPBinaryIVFRetrievalParameters() : RetrievalParameters(), nprobe_(-1) {}
  int Nprobe() { return nprobe_; }
  void SetNprobe(int nprobe) { nprobe_ = nprobe; }

 private:
  int nprobe_;   // -1: not set (Search takes the model's 20)
};

class GammaBinaryIVFHIPIndex : public RetrievalModel {
 public:
  GammaBinaryIVFHIPIndex() {}
  ~GammaBinaryIVFHIPIndex() override;
  int Init(const std::string &model_parameters, int indexing_size) override;
  RetrievalParameters *Parse(const std::string &parameters) override;
  int Indexing() override;
  bool Add(int n, const uint8_t *vec) override;
  int Update(const std::vector<int64_t> &ids, const std::vector<const uint8_t *> &vecs) override { return 0; }
  int Delete(const std::vector<int64_t> &ids) override;
  int Search(RetrievalContext *retrieval_context, int n, const uint8_t *x, int k, float *distances,
             int64_t *ids) override;
  long GetTotalMemBytes() override { return h_ ? (long)gamma_hip_total_mem_bytes(h_) : 0; }
  int Dump(const std::string &dir) override { return 0; }
  int Load(const std::string &dir) override { return 0; }

  int nlist_ = 256;
  int nprobe_ = 20;
  int nbits_ = 0;
  bool is_trained_ = false;

 private:
  int SyncVid2DocID(int64_t upto);
  int EnsureFlat(int64_t upto);   // brute_force_search / untrained model: the exact search's mirror of the store
  gamma_hip_index *h_ = nullptr;
  int64_t indexed_vec_count_ = 0;
  bool flat_init_ = false;       // (under add_mu_)
  int64_t flat_mirrored_ = 0;    // rows of the engine's store in the flat store (under add_mu_)
  std::mutex add_mu_;
  bool device_filters_ = false;
  DeviceColumns columns_;
};

}  // namespace tig_gamma
