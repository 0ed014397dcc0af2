// GammaIVFPQHIPIndex -- RetrievalModel plugin "HIPIVFPQ": Gamma's IVFPQ model with the whole
// search path (coarse quantizer, LUT, list scan, filters, top-k, re-rank) and the Add-path
// encoding on an MI355X through the C ABI of include/gamma_hip.h.
//
// Mirrors GammaIVFPQIndex (reference index/impl/gamma_index_ivfpq.{h,cc}): same JSON keys and
// defaults (the reference's IVFPQModelParams :675-887 and IVFPQRetrievalParameters :629-673), same
// return codes, same Search contract.  The parameter classes carry a HIP prefix: the plugin is compiled
// INTO libgamma next to the reference's own IVFPQ model, where a second
// tig_gamma::IVFPQModelParams with another layout would be an ODR violation.  Unsupported on device and rejected in Init like any bad parameter:
// hnsw quantizer, support_indivisible_nsubvector, opq together with several devices or 4-bit codes (opq itself: through the
// ops table that gamma_index_ivfpq_opq_hip.cc registers; trained in Indexing, carried by Dump / Load as the "LTra" record), nbits_per_idx other than 8 and 4 (4: one device only, through the
// lists initialiser that gamma_index_ivfpq4_hip.cc registers).
#pragma once
#include <atomic>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/gamma_hip.h"
#include "plugin_includes.h"
#include "filter_bridge.h"

namespace tig_gamma {

void WarnTiesNotHonoured(gamma_hip_index *h, gamma_hip_group *grp, std::atomic<int64_t> *said);
void WarnBlasCorners(gamma_hip_index *h, gamma_hip_group *grp, std::atomic<int64_t> *said);   // gamma_index_ivfpq_hip.cc

class HIPIVFPQRetrievalParameters : public RetrievalParameters {
 public:
  HIPIVFPQRetrievalParameters() : RetrievalParameters(), parallel_on_queries_(true), recall_num_(100), nprobe_(-1), exact_ties_(0) {}
  HIPIVFPQRetrievalParameters(enum DistanceComputeType type)
      : RetrievalParameters(type), parallel_on_queries_(true), recall_num_(100), nprobe_(-1), exact_ties_(0) {}
  int RecallNum() { return recall_num_; }
  void SetRecallNum(int recall_num) { recall_num_ = recall_num; }
  int Nprobe() { return nprobe_; }
  void SetNprobe(int nprobe) { nprobe_ = nprobe; }
  bool ParallelOnQueries() { return parallel_on_queries_; }
  void SetParallelOnQueries(bool p) { parallel_on_queries_ = p; }
  // HIP only ("exact_ties" in the request's retrieval parameters): 0 = the model's setting, 1 = on, -1 = off
  int ExactTies() { return exact_ties_; }
  void SetExactTies(int v) { exact_ties_ = v; }

 protected:
  bool parallel_on_queries_;   // accepted for compatibility; the device path is always batched
  int recall_num_;
  int nprobe_;
  int exact_ties_;
};

// Lists initialiser of an nbits_per_idx other than 8 (4: gamma_hip_ivfpq4_init).  The translation unit that carries the ABI
// call registers it at static-initialisation time, the idiom of REGISTER_MODEL; HIPIVFPQ::Init looks it up by
// nbits_per_idx and rejects the value where none is registered (a build without that unit).
typedef int (*HIPListsInitFn)(gamma_hip_index *h, int d, int nlist, int M, int metric, int bucket_init_size,
                              int bucket_max_size);
int RegisterHIPListsInit(int nbits, HIPListsInitFn fn);
HIPListsInitFn FindHIPListsInit(int nbits);

// "raw_placement": "sharded" (several devices, lists sharded): every raw row once, on the device that owns its list.  The ABI
// entries that takes beyond those of the replicated mirror -- the group's placement switch and row routing, the store's clear --
// are registered by gamma_index_ivfpq_rawshard_hip.cc at static-initialisation time (the idiom of RegisterHIPListsInit):
// builds of the plugin against a C ABI without them leave that file out, and HIPIVFPQ::Init then rejects the value.
struct HIPRawShardOps {
  int (*set_raw_placement)(gamma_hip_group *g, int sharded);
  int (*group_raw_put)(gamma_hip_group *g, int64_t n, const int64_t *vids, const float *vecs, int64_t *n_skipped);
  int (*raw_clear)(gamma_hip_index *h);
  // "raw_dtype": "float16" | "uint8" | "int8" beside it: the members' stores serve narrow rows sharded with their lists
  // (gamma_hip_set_sparse_narrow_rows)
  int (*narrow_rows)(gamma_hip_index *h, int on);
};
int RegisterHIPRawShard(const HIPRawShardOps *ops);
const HIPRawShardOps *FindHIPRawShard();

// "raw_dtype": "float16": the raw store's initialiser for rows of IEEE binary16 (gamma_hip_raw_init_f16), registered at
// static-initialisation time by gamma_index_ivfpq_rawf16_hip.cc -- the only host file that names it (the idiom of
// RegisterHIPListsInit).  A build of the plugin without that file has none, and HIPIVFPQ::Init rejects the value.
typedef int (*HIPRawInitFn)(gamma_hip_index *h, int d);
int RegisterHIPRawInitF16(HIPRawInitFn fn);
HIPRawInitFn FindHIPRawInitF16();
// "raw_dtype": "uint8" | "int8": the byte store's entries of the C ABI -- its initialiser (gamma_hip_raw_init_i8) and the
// writers' acceptance predicate (gamma_hip_raw_i8_check) -- registered the same way by gamma_index_ivfpq_rawi8_hip.cc, the only
// host file that names them.  Without that file Init rejects the two values.
struct HIPRawI8Ops {
  int (*init)(gamma_hip_index *h, int d, int is_signed);
  int (*check)(const float *x, int64_t n, int is_signed, int64_t *first_bad);
};
int RegisterHIPRawI8(const HIPRawI8Ops *ops);
const HIPRawI8Ops *FindHIPRawI8();
// The byte stores' rule in front of a model's writers (HIPIVFPQ and HIPFLAT): true when every value of the nrows x d rows converts
// exactly; otherwise one log line "[model] what refused: ..." naming row, element and value, and false -- before anything changes.
bool HIPRowsStorableI8(const HIPRawI8Ops *ops, bool is_signed, int d, const char *model, const char *what, const float *x,
                       int64_t nrows);
// "raw_dtype": "sq8": the scalar-quantised store's entries of the C ABI -- its initialiser, the ranges (set / get / train) and the
// writers' acceptance predicate -- registered the same way by gamma_index_ivfpq_rawsq8_hip.cc, the only host file that names
// them.  Without that file Init rejects the value.
struct HIPRawSq8Ops {
  int (*init)(gamma_hip_index *h, int d);
  int (*set_ranges)(gamma_hip_index *h, const float *vmin, const float *vmax);
  int (*get_ranges)(gamma_hip_index *h, float *vmin, float *vmax);
  int (*train)(gamma_hip_index *h, int64_t n, const float *x);
  int (*check)(const float *x, int64_t n, int64_t *first_bad);
};
int RegisterHIPRawSq8(const HIPRawSq8Ops *ops);
const HIPRawSq8Ops *FindHIPRawSq8();

// The "raw_dtype" key of the HIPFLAT and HIPIVFFLAT models' parameters: *et = 0 float32 (also: no key), 1 float16, 2 uint8, 3 int8,
// case-insensitive; any other string: one log line "[model] invalid raw_dtype = ..." and -1.
int HIPParseRawDtype(const char *model, const std::string &model_parameters, int *et);

// HIPIVFFLAT's "raw_dtype": "float16" | "uint8" | "int8": IVFFLAT search over narrow rows is a switch of the handle
// (gamma_hip_set_ivfflat_narrow_rows), registered the same way by gamma_index_ivfflat_rows_hip.cc, the only host file that names
// it.  Without that file HIPIVFFLAT::Init rejects the three values.
typedef int (*HIPIVFFlatRowsFn)(gamma_hip_index *h, int on);
int RegisterHIPIVFFlatRows(HIPIVFFlatRowsFn fn);
HIPIVFFlatRowsFn FindHIPIVFFlatRows();
// HIPIVFFLAT's "raw_dtype": "sq8" (with "sq8_ranges": "trained"): a switch of its own (gamma_hip_set_ivfflat_sq8_rows), registered
// by gamma_index_ivfflat_sq8_hip.cc -- the only host file that names it; the store's entries are HIPRawSq8Ops above.  Without
// either HIPIVFFLAT::Init rejects the value.
typedef int (*HIPIVFFlatSq8RowsFn)(gamma_hip_index *h, int on);
int RegisterHIPIVFFlatSq8Rows(HIPIVFFlatSq8RowsFn fn);
HIPIVFFlatSq8RowsFn FindHIPIVFFlatSq8Rows();

// HIPIVFFLAT with "devices": "0,1,.." (several): the in-process group's IVFFLAT search (gamma_hip_group_ivfflat_search), registered
// the same way by gamma_index_ivfflat_group_hip.cc -- the only host file that names it.  Without that file HIPIVFFLAT reads none of
// "devices" / "placement" / "raw_placement" and opens one handle, as it always did.
typedef int (*HIPIVFFlatGroupSearchFn)(gamma_hip_group *g, const gamma_hip_search_params *p, int nq, const float *x, int k,
                                       float *distances, int64_t *labels);
int RegisterHIPIVFFlatGroup(HIPIVFFlatGroupSearchFn fn);
HIPIVFFlatGroupSearchFn FindHIPIVFFlatGroup();
// HIPIVFFLAT's "group_rows": "float32" (the default: the members of a group hold fp32 rows, a narrow raw_dtype with several
// devices is rejected) | "raw_dtype" (the members hold their rows in raw_dtype: float16 / uint8 / int8).  The key's parser and the
// decision -- no device is touched -- live in gamma_index_ivfflat_group_rows_hip.cc and are registered the same way; without that
// file the key stays unread and the model behaves as it always did.  et: the parsed raw_dtype (0 float32 .. 4 sq8); ndevices /
// device_filters: the parsed "devices" / "device_filters".  0 accepted (*members_narrow = 1: the members get the typed store and
// the handles' switches), -2 rejected behind one log line.
typedef int (*HIPIVFFlatGroupRowsFn)(const std::string &model_parameters, int et, size_t ndevices, bool device_filters,
                                     int *members_narrow);
int RegisterHIPIVFFlatGroupRows(HIPIVFFlatGroupRowsFn fn);
HIPIVFFlatGroupRowsFn FindHIPIVFFlatGroupRows();

// "opq": the rotation's entries of the C ABI (gamma_hip_opq_train / _set / _get / _apply) reach the model through this table,
// registered at static-initialisation time by gamma_index_ivfpq_opq_hip.cc -- the only host file that names them.  A build of
// the plugin without that file (against a C ABI without those entries) has no table, and HIPIVFPQ::Init rejects "opq".
struct HIPOpqOps {
  int (*train)(gamma_hip_index *h, int d, int64_t n, const float *x, int M_opq, int niter, float *A, float *objective);
  int (*set)(gamma_hip_index *h, const float *A);
  int (*get)(gamma_hip_index *h, float *A);
  int (*apply)(gamma_hip_index *h, int64_t n, const float *x, float *xt);
};
int RegisterHIPOpq(const HIPOpqOps *ops);
const HIPOpqOps *FindHIPOpq();

struct HIPIVFPQModelParams {
  int ncentroids = 2048;
  int nsubvector = 64;
  bool support_indivisible_nsubvector = false;
  int nbits_per_idx = 8;
  int nprobe = 80;
  DistanceComputeType metric_type = DistanceComputeType::INNER_PRODUCT;
  bool has_hnsw = false;
  bool has_opq = false;
  int opq_nsubvector = 64;       // "opq": {"nsubvector": N} (gamma_index_ivfpq.h:835-847)
  int bucket_init_size = 1000;
  int bucket_max_size = 1280000;
  bool device_filters = false;   // HIP only: evaluate range / term filters on device-resident columns (filter_bridge.h)
  bool exact_ties = true;        // HIP only: the reference's heap order inside exact distance ties (gamma_hip_set_exact_ties)
  bool perf_stages = false;      // HIP only: per-stage device times in the request's PerfTool (stage events on every search)
  std::vector<int> devices;      // HIP only: "devices": "0,1,2,3" -- the index sharded by IVF list over these GPUs in this
                                 // process (gamma_hip_group_*); empty: one GPU, GAMMA_HIP_DEVICE or 0
  bool replicate = false;        // HIP only: "placement": "replicate" -- every device holds every list, a search splits
                                 // the queries (results of one GPU bit for bit); "shard" (default): by IVF list
  bool raw_sharded = false;      // HIP only: "raw_placement": "sharded" -- with several devices and list placement every raw
                                 // vector lives once, on the device that owns its list; "replicated" (default): on all
  bool raw_f16 = false;          // HIP only: "raw_dtype": "float16" -- the device's raw rows (what compute_dis reads) are IEEE
                                 // binary16, rounded from the engine's fp32 on upload; "float32" (default).  Several devices:
                                 // with "raw_placement": "sharded" only.
  int raw_i8 = 0;                // HIP only: "raw_dtype": "uint8" (1) | "int8" (2) -- the device's raw rows are one byte per
                                 // element; a row that does not convert exactly is refused by Add / Update.  Several devices:
                                 // with "raw_placement": "sharded" only (as "float16").
  bool raw_sq8 = false;          // HIP only: "raw_dtype": "sq8" -- the device's raw rows are one scalar-quantised byte per element
                                 // (lossy; ranges = per-dimension minimum / maximum of the training rows).  One device only.
  int Parse(const char *str);   // 0 ok, -1 bad (same rules as gamma_index_ivfpq.h:708-851)
  // "raw_placement" / "raw_dtype" against "devices" / "placement" and what this build of the plugin carries, as HIPIVFPQ::Init
  // decides it before a device is opened: 0 accepted, -2 rejected behind one log line
  int CheckRawKeys() const;
};

class GammaIVFPQHIPIndex : public RetrievalModel {
 public:
  GammaIVFPQHIPIndex();
  ~GammaIVFPQHIPIndex() override;
  int Init(const std::string &model_parameters, int indexing_size) override;
  RetrievalParameters *Parse(const std::string &parameters) override;
  int Indexing() override;
  bool Add(int n, const uint8_t *vec) override;
  int Update(const std::vector<int64_t> &ids, const std::vector<const uint8_t *> &vecs) override;
  int Delete(const std::vector<int64_t> &ids) override;
  int Search(RetrievalContext *retrieval_context, int n, const uint8_t *x, int k, float *distances,
             int64_t *ids) override;
  long GetTotalMemBytes() override;
  int Dump(const std::string &dir) override;
  int Load(const std::string &dir) override;

  // install an externally trained quantizer (tests: same centroids as the oracle)
  int SetTrained(const float *coarse_centroids, const float *pq_centroids);

  // exposed for the harness / tests
  int Sq8Ranges(float *vmin, float *vmax);   // "raw_dtype": "sq8": the store's ranges, d floats each; 1 has them, 0 not, -1 no sq8 model
  bool is_trained_ = false;
  int d_ = 0, nlist_ = 0, M_ = 0, nprobe_ = 80;
  DistanceComputeType metric_type_ = DistanceComputeType::INNER_PRODUCT;
  int indexed_vec_count_ = 0;
  std::vector<float> coarse_centroids_, pq_centroids_;
  std::vector<float> opq_A_;   // "opq": the trained / loaded rotation, d x d row-major (empty before training)

 protected:
  const HIPOpqOps *opq_ = nullptr;   // non-null: the model was created with "opq"
  int opq_M_ = 0;
  int TrainOnHost(size_t num, const float *xt);
  int TrainCoarse(size_t num, const float *xt);
  int TrainingSet(std::vector<float> &xt, size_t &num);
  int EnsureRaw(int64_t upto);
  int EnsureRawLocked(int64_t upto);   // raw_mu_ held
  int ShardRows();                     // "raw_placement": "sharded": member 0's dense mirror goes, the group takes the rows
  int PutRowsFromStore(int64_t upto);  // ... and after a Load gets them from the engine's vector store
  int UploadEngineBitmap();
  int SyncVid2DocID(int64_t upto);   // multi-vector documents: docids of vids [0, upto) to the device (VIDMgr)
  std::mutex raw_mu_;   // raw_uploaded_ + the mirror writes (Search threads, the indexing thread, Load)
  DeviceColumns columns_;
  // one GPU: h_ alone.  "devices" with several entries: a group of handles, lists sharded by owner; h_ is member 0 and
  // serves what needs no lists (training's assignment step, brute-force search over the replicated raw vectors)
  gamma_hip_group *grp_ = nullptr;
  std::vector<gamma_hip_index *> members_;   // where replicated state goes: {h_} or every member of the group
  template <typename F>
  int ForAll(F f) {
    for (gamma_hip_index *m : members_) {
      const int rc = f(m);
      if (rc) return rc;
    }
    return 0;
  }
  int OpenDevices(const std::vector<int> &devices, bool replicate = false);
  void PerfLabels(GammaSearchCondition *cond);
  std::mutex perf_mu_;
  double perf_ms_[GAMMA_HIP_NUM_STAGES] = {0};
  gamma_hip_index *h_ = nullptr;
  std::atomic<int64_t> blas_said_{0};   // WarnBlasCorners
  std::atomic<int64_t> ties_said_{0};   // WarnTiesNotHonoured: what this model has reported so far
  HIPIVFPQModelParams *model_param_ = nullptr;
  int64_t raw_uploaded_ = 0;
  // "raw_placement": "sharded".  Until the first Add after training (or a Load) member 0 alone mirrors the vector store by
  // vid, for the brute-force search of an untrained model; from then on (rows_sharded_) the group keeps every row at the
  // owner of its list, Add and Update hand the rows to the group, and a brute-force request is refused.
  const HIPRawShardOps *rawshard_ = nullptr;
  bool raw_f16_ = false;               // "raw_dtype": "float16": no device holds fp32 rows -- brute-force search is refused
  int raw_i8_ = 0;                     // "raw_dtype": "uint8" (1) | "int8" (2): likewise
  const HIPRawI8Ops *raw_i8_ops_ = nullptr;
  bool RowsStorable(const char *what, const float *x, int64_t nrows);   // byte / sq8 store (float16: where the rows are sharded): one log line for the first refused value
  // "raw_dtype": "sq8": likewise.  The ranges are trained by Indexing() before the first row is mirrored, written by Dump to the
  // side file raw_sq8.ranges beside ivfpq.index (HIPIVFFLAT: ivfflat.index) and set again by Load before the mirror is re-encoded.
  const HIPRawSq8Ops *raw_sq8_ops_ = nullptr;
  int DumpSq8Ranges(const std::string &index_dir);
  int LoadSq8Ranges(const std::string &index_dir);
  bool rows_sharded_ = false;          // under raw_mu_
  // nbits_per_idx: 8, or 4 (16 centroids per sub-quantizer, two indices per code byte as faiss's PQEncoderGeneric packs them)
  int nbits_ = 8;
  size_t Ksub() const { return (size_t)1 << nbits_; }
  size_t CodeSize() const { return ((size_t)nbits_ * M_ + 7) / 8; }
};

// "HIPIVFFLAT": the reference's IVFFLAT model (index/impl/gamma_index_ivfflat.{h,cc}) on the device.  Same JSON
// keys (ncentroids, nprobe, metric_type; retrieval: metric_type, nprobe, parallel_on_queries), same Search
// contract.  The reference keeps the vectors inside the inverted lists; here the lists hold vector ids and the rows
// come from the HBM mirror of the vector store the IVFPQ plugin already keeps for its re-rank, so Add / Update /
// Delete and the raw mirror are inherited; Init, Indexing (coarse k-means only), Search, Dump / Load ("IvFl" file,
// iwpq_io.h) differ.
// HIP only: "devices": "0,1,..", "placement": "shard" | "replicate", "raw_placement": "replicated" | "sharded" with HIPIVFPQ's
// meaning -- the index on several GPUs of this process (gamma_hip_group_*), no device_filters; fp32 rows, or with "group_rows":
// "raw_dtype" the members' rows in a raw_dtype of float16 / uint8 / int8 (HIPIVFFlatGroupRowsFn above).
// HIP only: "raw_dtype": "float32" (default) | "float16" | "uint8" | "int8" -- the device's rows are 2 bytes / 1 byte per element,
// widened exactly as the scan loads them; the byte stores take a row only if it converts exactly (HIPIVFPQ's rule, inherited).
// Unlike HIPIVFPQ the model serves brute_force_search and the search of an untrained model over a narrow store (flat search
// over narrow rows, gamma_index_flat_hip.h) where the build has that switch.
class HIPIVFFlatRetrievalParameters : public RetrievalParameters {
 public:
  HIPIVFFlatRetrievalParameters() : RetrievalParameters(), parallel_on_queries_(true), nprobe_(-1), exact_ties_(0) {}
  HIPIVFFlatRetrievalParameters(enum DistanceComputeType type)
      : RetrievalParameters(type), parallel_on_queries_(true), nprobe_(-1), exact_ties_(0) {}
  int Nprobe() { return nprobe_; }
  // HIP only ("exact_ties" in the request's retrieval parameters): 0 = the model's setting, 1 = on, -1 = off
  int ExactTies() { return exact_ties_; }
  void SetExactTies(int v) { exact_ties_ = v; }
  void SetNprobe(int nprobe) { nprobe_ = nprobe; }
  bool ParallelOnQueries() { return parallel_on_queries_; }
  void SetParallelOnQueries(bool p) { parallel_on_queries_ = p; }

 protected:
  bool parallel_on_queries_;   // accepted for compatibility; the device path is always batched
  int nprobe_;
  int exact_ties_;
};

class GammaIVFFlatHIPIndex : public GammaIVFPQHIPIndex {
 public:
  int Init(const std::string &model_parameters, int indexing_size) override;
  RetrievalParameters *Parse(const std::string &parameters) override;
  int Indexing() override;
  int Search(RetrievalContext *retrieval_context, int n, const uint8_t *x, int k, float *distances,
             int64_t *ids) override;
  int Dump(const std::string &dir) override;
  int Load(const std::string &dir) override;
  int SetTrainedCoarse(const float *coarse_centroids);
  // the "raw_dtype" key of the model's parameters: HIPParseRawDtype's answer, and *et = 4 for "sq8" together with
  // "sq8_ranges": "trained" (case-insensitive; the ranges are learned by Indexing() and kept in raw_sq8.ranges beside
  // ivfflat.index).  -1 and one log line for "sq8" without that key (as before), any other value of the key, the key beside
  // another raw_dtype, and sq8_min / sq8_max (HIPFLAT's keys: this model's ranges are per dimension and trained)
  static int ParseRawDtype(const std::string &model_parameters, int *et);
  // What Init says to "devices" / "placement" / "raw_placement" / "group_rows" beside raw_dtype (et) and pa.device_filters, before
  // a device is opened: 0 accepted (pa takes the device keys; *several: a group is opened; *members_narrow: its members hold
  // rows of raw_dtype), -1 rejected behind one log line.  In a build without the group's IVFFLAT search none of the keys is read.
  static int DeviceKeys(const std::string &model_parameters, int et, HIPIVFPQModelParams &pa, bool *several, bool *members_narrow);
  // the same from the model's parameters alone (the harness): out = {rc of the raw_dtype / device keys' parsing and the decision,
  // several, members_narrow}
  static void CheckGroupKeys(const std::string &model_parameters, int *out);

 private:
  HIPIVFFlatGroupSearchFn group_search_ = nullptr;   // non-null: the build carries the group's IVFFLAT search
  bool narrow_brute_ = true;   // false: a narrow store in a build without flat search over narrow rows -- brute force is refused
};

}  // namespace tig_gamma
