// GammaFLATHIPIndex -- RetrievalModel plugin "HIPFLAT": Gamma's brute-force model
// (reference index/impl/gamma_index_flat.{h,cc}) on an MI355X.  Same JSON keys
// (metric_type, parallel_on_queries), same Search contract.
// HIP only: "raw_dtype": "float32" (the default) | "float16" | "uint8" | "int8" -- the element type of the device's rows, which
// ARE the index.  Results are those of the fp32 model over the widened rows; a byte model accepts a row only if every value
// converts exactly (HIPIVFPQ's rule), a float16 model rounds and refuses an overflow.
// "raw_dtype": "sq8" with "sq8_min": <number> and "sq8_max": <number> (both required, and only with sq8): rows of one
// scalar-quantised byte per element, ONE range for every dimension -- a flat model has no training step in which ranges could be
// learned.  Results are those of the fp32 model over the decoded rows; a row is accepted only if every value is finite.
#pragma once
#include <atomic>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/gamma_hip.h"
#include "plugin_includes.h"
#include "filter_bridge.h"

namespace tig_gamma {

struct HIPRawI8Ops;   // gamma_index_ivfpq_hip.h
struct HIPRawSq8Ops;  // gamma_index_ivfpq_hip.h
// Flat search over narrow rows is a switch of the handle (gamma_hip_set_flat_narrow_rows), registered at static-initialisation
// time by gamma_index_flat_rows_hip.cc -- the only host file that names it (the idiom of RegisterHIPRawI8).  A build of the plugin
// without that file (against a C ABI without the entry) has none, and HIPFLAT::Init rejects a narrow "raw_dtype".
typedef int (*HIPFlatRowsFn)(gamma_hip_index *h, int on);
int RegisterHIPFlatRows(HIPFlatRowsFn fn);
HIPFlatRowsFn FindHIPFlatRows();
// The same for an sq8 store: a switch of its own (gamma_hip_set_flat_sq8_rows), registered by gamma_index_flat_sq8_hip.cc -- the
// only host file that names it.  Without that file HIPFLAT::Init rejects "raw_dtype": "sq8".
typedef int (*HIPFlatSq8RowsFn)(gamma_hip_index *h, int on);
int RegisterHIPFlatSq8Rows(HIPFlatSq8RowsFn fn);
HIPFlatSq8RowsFn FindHIPFlatSq8Rows();

class HIPFlatRetrievalParameters : public RetrievalParameters {
 public:
  HIPFlatRetrievalParameters() : RetrievalParameters(), parallel_on_queries_(true), exact_ties_(0) {}
  HIPFlatRetrievalParameters(bool parallel_on_queries, enum DistanceComputeType type)
      : RetrievalParameters(type), parallel_on_queries_(parallel_on_queries), exact_ties_(0) {}
  HIPFlatRetrievalParameters(enum DistanceComputeType type) : RetrievalParameters(type), parallel_on_queries_(true), exact_ties_(0) {}
  bool ParallelOnQueries() { return parallel_on_queries_; }
  // HIP only ("exact_ties" in the request's retrieval parameters): 0 = the model's setting, 1 = on, -1 = off
  int ExactTies() { return exact_ties_; }
  void SetExactTies(int v) { exact_ties_ = v; }

 private:
  bool parallel_on_queries_;   // accepted for compatibility; the device path is always batched
  int exact_ties_;
};

class GammaFLATHIPIndex : public RetrievalModel {
 public:
  GammaFLATHIPIndex() {}
  ~GammaFLATHIPIndex() override;
  int Init(const std::string &model_parameters, int indexing_size) override;
  RetrievalParameters *Parse(const std::string &parameters) override;
  int Indexing() override { return 0; }
  bool Add(int n, const uint8_t *vec) override;
  int Update(const std::vector<int64_t> &ids, const std::vector<const uint8_t *> &vecs) override;
  int Delete(const std::vector<int64_t> &ids) override;
  int Search(RetrievalContext *retrieval_context, int n, const uint8_t *x, int k, float *distances,
             int64_t *ids) override;
  long GetTotalMemBytes() override { return h_ ? (long)gamma_hip_total_mem_bytes(h_) : 0; }
  int Dump(const std::string &dir) override { return 0; }
  int Load(const std::string &dir) override;
  DistanceComputeType metric_type_ = DistanceComputeType::INNER_PRODUCT;
  // the "raw_dtype" key of the model parameters: *et = 0 float32 (also when the key is absent), 1 float16, 2 uint8, 3 int8
  // (gamma_hip_raw_elem_type), 4 sq8 with its range in sq8_range[2] = {sq8_min, sq8_max} (if given); -1, one log line and
  // *et = 0 for any other string, parameters that do not parse, sq8 without both of its keys as numbers, a bound that is not
  // finite as a float, sq8_min > sq8_max or a span that is not finite, and for either key beside another raw_dtype
  static int ParseRawDtype(const std::string &model_parameters, int *et, float *sq8_range = nullptr);

 private:
  int raw_et_ = 0;
  const HIPRawI8Ops *raw_i8_ops_ = nullptr;
  const HIPRawSq8Ops *raw_sq8_ops_ = nullptr;
  bool RowsStorable(const char *what, const float *x, int64_t nrows);   // byte rows: every value converts exactly; sq8: is finite
  gamma_hip_index *h_ = nullptr;
  std::atomic<int64_t> ties_said_{0};   // WarnTiesNotHonoured: what this model has reported so far
  int d_ = 0;
  int64_t uploaded_ = 0;
  int SyncVid2DocID(int64_t upto);
  std::mutex raw_mu_;   // uploaded_ + the mirror writes
  bool device_filters_ = false;
  bool exact_ties_ = true;      // "exact_ties" of the model parameters (HIP only, default on)
  DeviceColumns columns_;
};

}  // namespace tig_gamma
