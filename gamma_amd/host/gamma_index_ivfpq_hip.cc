// GammaIVFPQHIPIndex -- see gamma_index_ivfpq_hip.h.  Host side only: parameter handling,
// training driver, bookkeeping; every distance / scan / selection runs in libgamma_hip.so.
#include "gamma_index_ivfpq_hip.h"
#include "gamma_index_flat_hip.h"   // FindHIPFlatRows (HIPIVFFLAT over a narrow store: brute force)

#include "iwpq_io.h"

#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <strings.h>
#include <sys/stat.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <random>

namespace tig_gamma {

REGISTER_MODEL(HIPIVFPQ, GammaIVFPQHIPIndex);

#define HLOG(...)                      \
  do {                                 \
    fprintf(stderr, "[HIPIVFPQ] ");    \
    fprintf(stderr, __VA_ARGS__);      \
    fprintf(stderr, "\n");             \
  } while (0)

// "devices", "placement", "raw_placement": the keys HIPIVFPQ and HIPIVFFLAT share, one meaning and one parser
static int ParseDeviceKeys(utils::JsonParser &jp, HIPIVFPQModelParams &pa) {
  int v = 0;
  std::string devs;
  if (!jp.GetString("devices", devs)) {   // "0,1,2,3" (the engine's JsonParser has no arrays)
    pa.devices.clear();
    size_t at = 0;
    while (at < devs.size()) {
      size_t end = devs.find(',', at);
      if (end == std::string::npos) end = devs.size();
      const std::string tok = devs.substr(at, end - at);
      char *rest = nullptr;
      const long dv = strtol(tok.c_str(), &rest, 10);
      if (tok.empty() || (rest && *rest != '\0' && *rest != ' ') || dv < 0) {
        HLOG("invalid devices = %s", devs.c_str());
        return -1;
      }
      pa.devices.push_back((int)dv);
      at = end + 1;
    }
  } else if (!jp.GetInt("devices", v)) {   // a single ordinal
    if (v < 0) return -1;
    pa.devices.assign(1, v);
  }
  std::string plc;
  if (!jp.GetString("placement", plc)) {   // several devices: "shard" (by IVF list, the default) | "replicate"
    if (strcasecmp("shard", plc.c_str()) && strcasecmp("replicate", plc.c_str())) {
      HLOG("invalid placement = %s", plc.c_str());
      return -1;
    }
    pa.replicate = !strcasecmp("replicate", plc.c_str());
  }
  std::string rpl;
  if (!jp.GetString("raw_placement", rpl)) {   // several devices, lists sharded: "replicated" (the default) | "sharded"
    if (strcasecmp("replicated", rpl.c_str()) && strcasecmp("sharded", rpl.c_str())) {
      HLOG("invalid raw_placement = %s", rpl.c_str());
      return -1;
    }
    pa.raw_sharded = !strcasecmp("sharded", rpl.c_str());
  }
  return 0;
}

int HIPIVFPQModelParams::Parse(const char *str) {
  utils::JsonParser jp;
  if (jp.Parse(str)) {
    HLOG("parse IVFPQ retrieval parameters error: %s", str);
    return -1;
  }
  int v;
  if (!jp.GetInt("ncentroids", v)) {
    if (v < -1) return -1;
    if (v > 0) ncentroids = v;
  } else {
    HLOG("cannot get ncentroids for ivfpq, set it when create space");
    return -1;
  }
  if (!jp.GetInt("nsubvector", v)) {
    if (v < -1) return -1;
    if (v > 0) nsubvector = v;
  } else {
    HLOG("cannot get nsubvector for ivfpq, set it when create space");
    return -1;
  }
  if (!jp.GetInt("nbits_per_idx", v)) {
    if (v < -1) return -1;
    if (v > 0) nbits_per_idx = v;
  }
  if (!jp.GetInt("nprobe", v)) {
    if (v < -1) return -1;
    if (v > 0) nprobe = v;
    if (nprobe > ncentroids) {
      HLOG("nprobe should less than ncentroids");
      return -1;
    }
  }
  if (!jp.GetInt("support_indivisible_nsubvector", v)) support_indivisible_nsubvector = v != 0;
  if (!jp.GetInt("device_filters", v)) device_filters = v != 0;
  if (!jp.GetInt("exact_ties", v)) exact_ties = v != 0;
  if (!jp.GetInt("perf_stages", v)) perf_stages = v != 0;
  if (ParseDeviceKeys(jp, *this)) return -1;
  std::string rdt;
  if (!jp.GetString("raw_dtype", rdt)) {   // the device's raw rows: "float32" (the default) | "float16" | "uint8" | "int8" | "sq8"
    if (strcasecmp("float32", rdt.c_str()) && strcasecmp("float16", rdt.c_str()) && strcasecmp("uint8", rdt.c_str()) &&
        strcasecmp("int8", rdt.c_str()) && strcasecmp("sq8", rdt.c_str())) {
      HLOG("invalid raw_dtype = %s", rdt.c_str());
      return -1;
    }
    raw_f16 = !strcasecmp("float16", rdt.c_str());
    raw_i8 = !strcasecmp("uint8", rdt.c_str()) ? 1 : !strcasecmp("int8", rdt.c_str()) ? 2 : 0;
    raw_sq8 = !strcasecmp("sq8", rdt.c_str());
  }
  if (!jp.GetInt("bucket_init_size", v)) {
    if (v < -1) return -1;
    if (v > 0) bucket_init_size = v;
  }
  if (!jp.GetInt("bucket_max_size", v)) {
    if (v < -1) return -1;
    if (v > 0) bucket_max_size = v;
  }
  std::string mt;
  if (!jp.GetString("metric_type", mt)) {
    if (strcasecmp("L2", mt.c_str()) && strcasecmp("InnerProduct", mt.c_str())) {
      HLOG("invalid metric_type = %s", mt.c_str());
      return -1;
    }
    metric_type = !strcasecmp("L2", mt.c_str()) ? DistanceComputeType::L2 : DistanceComputeType::INNER_PRODUCT;
  }
  utils::JsonParser sub;
  has_hnsw = !jp.GetObject("hnsw", sub);
  has_opq = !jp.GetObject("opq", sub);
  if (has_opq && !sub.GetInt("nsubvector", v)) {   // gamma_index_ivfpq.h:835-847: default 64 (-1 keeps it)
    if (v <= 0 && v != -1) {
      HLOG("invalid opq_nsubvector = %d", v);
      return -1;
    }
    if (v > 0) opq_nsubvector = v;
  }
  if (ncentroids <= 0 || nsubvector <= 0 || nbits_per_idx <= 0) return -1;
  return 0;
}

// What "raw_placement" and "raw_dtype" ask of the devices, decided before one is opened: 0, or -2 behind one log line.
// A narrow raw_dtype goes with several devices only where the rows are sharded with their lists (the members' sparse stores
// convert: gamma_hip_set_sparse_narrow_rows); replicated rows are fp32, and sq8 keeps to one device (its trained ranges would
// have to reach every member).
int HIPIVFPQModelParams::CheckRawKeys() const {
  const HIPRawShardOps *rawshard = raw_sharded ? FindHIPRawShard() : nullptr;
  if (raw_sharded && (devices.size() < 2 || replicate || !rawshard)) {
    HLOG("raw_placement = sharded needs several devices and placement = shard%s",
         rawshard ? "" : " (and this build of the plugin carries no sharded raw rows)");
    return -2;
  }
  const bool several = devices.size() > 1 && !rawshard;   // several devices whose rows are replicated
  const HIPRawInitFn raw_init_f16 = raw_f16 ? FindHIPRawInitF16() : nullptr;
  if (raw_f16 && (!raw_init_f16 || several)) {
    HLOG("raw_dtype = float16 %s", raw_init_f16 ? "with several devices is not supported (the group's members hold fp32 rows)"
                                                : "is not supported by this build of the plugin (it carries no float16 raw store)");
    return -2;
  }
  const HIPRawI8Ops *raw_i8_ops = raw_i8 ? FindHIPRawI8() : nullptr;
  if (raw_i8 && (!raw_i8_ops || several)) {
    HLOG("raw_dtype = %s %s", raw_i8 == 2 ? "int8" : "uint8",
         raw_i8_ops ? "with several devices is not supported (the group's members hold fp32 rows)"
                     : "is not supported by this build of the plugin (it carries no 8-bit raw store)");
    return -2;
  }
  const HIPRawSq8Ops *raw_sq8_ops = raw_sq8 ? FindHIPRawSq8() : nullptr;
  if (raw_sq8 && (!raw_sq8_ops || devices.size() > 1)) {
    HLOG("raw_dtype = sq8 %s", raw_sq8_ops ? "with several devices is not supported (the group's members hold fp32 rows)"
                                           : "is not supported by this build of the plugin (it carries no sq8 raw store)");
    return -2;
  }
  return 0;
}

namespace {
struct ListsInitEntry {
  int nbits;
  HIPListsInitFn fn;
};
// (a function-local static: registrations run during static initialisation, in any order)
std::vector<ListsInitEntry> &ListsInits() {
  static std::vector<ListsInitEntry> v;
  return v;
}
const HIPRawShardOps *&RawShardOps() {
  static const HIPRawShardOps *ops = nullptr;
  return ops;
}
}  // namespace

int RegisterHIPRawShard(const HIPRawShardOps *ops) {
  RawShardOps() = ops;
  return 0;
}

const HIPRawShardOps *FindHIPRawShard() { return RawShardOps(); }

namespace {
const HIPOpqOps *&OpqOps() {
  static const HIPOpqOps *ops = nullptr;
  return ops;
}
}  // namespace
int RegisterHIPOpq(const HIPOpqOps *ops) {
  OpqOps() = ops;
  return 0;
}
const HIPOpqOps *FindHIPOpq() { return OpqOps(); }

namespace {
HIPRawInitFn &RawInitF16() {
  static HIPRawInitFn fn = nullptr;
  return fn;
}
}  // namespace
int RegisterHIPRawInitF16(HIPRawInitFn fn) {
  RawInitF16() = fn;
  return 0;
}
HIPRawInitFn FindHIPRawInitF16() { return RawInitF16(); }

namespace {
const HIPRawI8Ops *&RawI8Ops() {
  static const HIPRawI8Ops *ops = nullptr;
  return ops;
}
}  // namespace
int RegisterHIPRawI8(const HIPRawI8Ops *ops) {
  RawI8Ops() = ops;
  return 0;
}
const HIPRawI8Ops *FindHIPRawI8() { return RawI8Ops(); }

namespace {
const HIPRawSq8Ops *&RawSq8Ops() {
  static const HIPRawSq8Ops *ops = nullptr;
  return ops;
}
}  // namespace
int RegisterHIPRawSq8(const HIPRawSq8Ops *ops) {
  RawSq8Ops() = ops;
  return 0;
}
const HIPRawSq8Ops *FindHIPRawSq8() { return RawSq8Ops(); }

int RegisterHIPListsInit(int nbits, HIPListsInitFn fn) {
  ListsInits().push_back({nbits, fn});
  return 0;
}

HIPListsInitFn FindHIPListsInit(int nbits) {
  for (const ListsInitEntry &e : ListsInits())
    if (e.nbits == nbits) return e.fn;
  return nullptr;
}

GammaIVFPQHIPIndex::GammaIVFPQHIPIndex() {}

GammaIVFPQHIPIndex::~GammaIVFPQHIPIndex() {
  if (grp_) gamma_hip_group_destroy(grp_);   // owns its members, h_ among them
  else if (h_) gamma_hip_destroy(h_);
  delete model_param_;
}

// one handle, or a group of handles with the lists sharded by owner (gamma_hip_group_*; what the reference's GPU model
// does with IndexShards, index/impl/gpu/gamma_gpu_cloner.cpp:200-269)
int GammaIVFPQHIPIndex::OpenDevices(const std::vector<int> &devices, bool replicate) {
  if (devices.size() > 1) {
    int rc = gamma_hip_group_create(devices.data(), (int)devices.size(), &grp_);
    if (!rc) rc = gamma_hip_group_set_placement(grp_, replicate ? 1 : 0);
    if (rc) {
      HLOG("gamma_hip_group_create failed: %s", gamma_hip_strerror(rc));
      return -1;
    }
    for (int i = 0; i < gamma_hip_group_size(grp_); i++) members_.push_back(gamma_hip_group_member(grp_, i));
    h_ = members_[0];
    return 0;
  }
  const char *dev = getenv("GAMMA_HIP_DEVICE");
  const int ordinal = devices.size() == 1 ? devices[0] : (dev ? atoi(dev) : 0);
  int rc = gamma_hip_create(ordinal, &h_);
  if (rc) {
    HLOG("gamma_hip_create failed: %s", gamma_hip_strerror(rc));
    return -1;
  }
  members_.assign(1, h_);
  return 0;
}

int GammaIVFPQHIPIndex::Init(const std::string &model_parameters, int indexing_size) {
  indexing_size_ = indexing_size;
  model_param_ = new HIPIVFPQModelParams();
  HIPIVFPQModelParams &pa = *model_param_;
  if (model_parameters != "" && pa.Parse(model_parameters.c_str())) return -1;
  if (!vector_) {
    HLOG("vector_ must be set before Init");
    return -1;
  }
  d_ = vector_->MetaInfo()->Dimension();
  if (d_ % pa.nsubvector != 0) {
    HLOG("Dimension [%d] cannot divide by nsubvector [%d] (support_indivisible_nsubvector is not "
         "available on the HIP path)", d_, pa.nsubvector);
    return -2;
  }
  // nbits_per_idx other than 8: through a registered lists initialiser (4: gamma_index_ivfpq4_hip.cc), else rejected
  const HIPListsInitFn lists_init = pa.nbits_per_idx == 8 ? nullptr : FindHIPListsInit(pa.nbits_per_idx);
  opq_ = pa.has_opq ? FindHIPOpq() : nullptr;
  if (pa.has_hnsw || (pa.has_opq && !opq_) || pa.support_indivisible_nsubvector || (pa.nbits_per_idx != 8 && !lists_init)) {
    HLOG("hnsw / padded dimensions / nbits_per_idx other than 8 and 4%s are not supported by HIPIVFPQ",
         pa.has_opq && !opq_ ? " / opq (this build of the plugin carries no OPQ entries)" : "");
    return -2;
  }
  if (opq_) {
    if (d_ % pa.opq_nsubvector != 0) {   // gamma_index_ivfpq.cc:158-163
      HLOG("%d %% %d != 0, opq nsubvector should be divisible by dimension.", d_, pa.opq_nsubvector);
      return -2;
    }
    if (pa.devices.size() > 1 || pa.nbits_per_idx != 8) {
      HLOG("opq with several devices or with nbits_per_idx = 4 is not supported");
      return -2;
    }
    opq_M_ = pa.opq_nsubvector;
  }
  if (lists_init && pa.devices.size() > 1) {
    HLOG("nbits_per_idx = %d with several devices is not supported (the group of handles is 8-bit only)", pa.nbits_per_idx);
    return -2;
  }
  nbits_ = pa.nbits_per_idx;
  nlist_ = pa.ncentroids;
  M_ = pa.nsubvector;
  metric_type_ = pa.metric_type;
  nprobe_ = pa.nprobe;
  if (pa.devices.size() > 1 && pa.device_filters) {
    HLOG("device_filters with several devices is not supported (the columns live on one handle)");
    return -2;
  }
  if (const int krc = pa.CheckRawKeys()) return krc;   // "raw_placement" / "raw_dtype" against the devices and this build
  rawshard_ = pa.raw_sharded ? FindHIPRawShard() : nullptr;
  const HIPRawInitFn raw_init_f16 = pa.raw_f16 ? FindHIPRawInitF16() : nullptr;
  raw_f16_ = pa.raw_f16;
  const HIPRawI8Ops *raw_i8_ops = pa.raw_i8 ? FindHIPRawI8() : nullptr;
  raw_i8_ = pa.raw_i8;
  raw_i8_ops_ = raw_i8_ops;
  const HIPRawSq8Ops *raw_sq8_ops = pa.raw_sq8 ? FindHIPRawSq8() : nullptr;
  raw_sq8_ops_ = raw_sq8_ops;
  if (OpenDevices(pa.devices, pa.replicate)) return -1;
  int rc = ForAll([&](gamma_hip_index *m) {
    const int metric = metric_type_ == DistanceComputeType::L2 ? GAMMA_HIP_METRIC_L2 : GAMMA_HIP_METRIC_IP;
    int r = lists_init ? lists_init(m, d_, nlist_, M_, metric, pa.bucket_init_size, pa.bucket_max_size)
                       : gamma_hip_ivfpq_init(m, d_, nlist_, M_, 8, metric, pa.bucket_init_size, pa.bucket_max_size);
    if (!r) r = raw_sq8_ops ? raw_sq8_ops->init(m, d_) : raw_i8_ops ? raw_i8_ops->init(m, d_, pa.raw_i8 == 2) : raw_init_f16 ? raw_init_f16(m, d_) : gamma_hip_raw_init(m, d_);
    if (!r && rawshard_ && (raw_init_f16 || raw_i8_ops)) r = rawshard_->narrow_rows(m, 1);
    if (!r) r = gamma_hip_set_exact_ties(m, pa.exact_ties ? 1 : 0);
    if (!r && pa.perf_stages) r = gamma_hip_profile_enable(m, 1);
    return r;
  });
  if (rc) {
    HLOG("device init failed: %s (%s)", gamma_hip_strerror(rc), gamma_hip_last_error(h_));
    return -1;
  }
  // what IndexIVFPQ::precompute_table prints in verbose mode (faiss:IndexIVFPQ.cpp:443-448): never silent
  if (gamma_hip_ivfpq_use_precomputed_table(h_) == 0)
    HLOG("not precomputing table, it would be too big: %lld bytes (max %lld) -- L2 searches score with residual tables "
         "(use_precomputed_table = 0)", (long long)nlist_ * M_ * 1024, (long long)gamma_hip_get_precomputed_table_max_bytes());
  return 0;
}

RetrievalParameters *GammaIVFPQHIPIndex::Parse(const std::string &parameters) {
  if (parameters == "") return new HIPIVFPQRetrievalParameters(metric_type_);
  utils::JsonParser jp;
  if (jp.Parse(parameters.c_str())) {
    HLOG("parse retrieval parameters error: %s", parameters.c_str());
    return nullptr;
  }
  HIPIVFPQRetrievalParameters *rp = new HIPIVFPQRetrievalParameters();
  std::string mt;
  if (!jp.GetString("metric_type", mt)) {
    rp->SetDistanceComputeType(!strcasecmp("L2", mt.c_str()) ? DistanceComputeType::L2
                                                              : DistanceComputeType::INNER_PRODUCT);
  } else {
    rp->SetDistanceComputeType(metric_type_);
  }
  int v;
  if (!jp.GetInt("recall_num", v) && v > 0) rp->SetRecallNum(v);
  if (!jp.GetInt("nprobe", v) && v > 0) rp->SetNprobe(v);
  if (!jp.GetInt("parallel_on_queries", v)) rp->SetParallelOnQueries(v != 0);
  if (!jp.GetInt("exact_ties", v)) rp->SetExactTies(v != 0 ? 1 : -1);   // HIP only: this request's choice
  return rp;
}

// Training = faiss's, on the device (gamma_hip_kmeans: faiss::Clustering::train -- subsampling, rand_perm seeds,
// centroid sums, empty-cluster splits -- with the assignment and the sums on the GPU, the training set resident).
int GammaIVFPQHIPIndex::TrainCoarse(size_t num, const float *xt) {
  // IndexIVF::train_q1: Clustering(d, nlist, cp) with cp.niter = 10 (gamma_index_ivfpq.cc:175), seed 1234,
  // max_points_per_centroid 256
  coarse_centroids_.resize((size_t)nlist_ * d_);
  return gamma_hip_kmeans(h_, d_, (int64_t)num, xt, nlist_, 10, 1234, 256, coarse_centroids_.data(), nullptr);
}

int GammaIVFPQHIPIndex::TrainOnHost(size_t num, const float *xt) {
  // IndexIVFPQ::train (train_q1 + train_residual_o + ProductQuantizer::train) on the device: gamma_hip_ivfpq_train
  coarse_centroids_.resize((size_t)nlist_ * d_);
  pq_centroids_.resize((size_t)M_ * Ksub() * (d_ / M_));
  return gamma_hip_ivfpq_train(h_, d_, (int64_t)num, xt, nlist_, M_, coarse_centroids_.data(), pq_centroids_.data());
}

int GammaIVFPQHIPIndex::Indexing() {
  if (is_trained_) {
    HLOG("already trained, skip indexing");
    return 0;
  }
  std::vector<float> xt;
  size_t num = 0;
  if (TrainingSet(xt, num)) return -1;
  int rc = 0;
  if (raw_sq8_ops_) {
    // "raw_dtype": "sq8": the store's ranges from the training rows (as the engine holds them: the store keeps the caller's rows,
    // not the rotated ones), before any row is mirrored -- a narrow store's mirror is written from Add on
    rc = raw_sq8_ops_->train(h_, (int64_t)num, xt.data());
    if (rc) {
      HLOG("sq8 range training failed: %s (%s)", gamma_hip_strerror(rc), gamma_hip_last_error(h_));
      return -1;
    }
  }
  if (opq_) {   // gamma_index_ivfpq.cc:336-346: train the rotation, then everything else on the rotated set
    opq_A_.resize((size_t)d_ * d_);
    std::vector<float> rot(xt.size());
    rc = opq_->train(h_, d_, (int64_t)num, xt.data(), opq_M_, 0, opq_A_.data(), nullptr);
    if (!rc) rc = opq_->set(h_, opq_A_.data());
    if (!rc) rc = opq_->apply(h_, (int64_t)num, xt.data(), rot.data());
    if (rc) {
      HLOG("opq training failed: %s (%s)", gamma_hip_strerror(rc), gamma_hip_last_error(h_));
      opq_A_.clear();
      return -1;
    }
    xt.swap(rot);
  }
  if (!rc) rc = TrainOnHost(num, xt.data());
  if (!rc) rc = ForAll([&](gamma_hip_index *m) {
    return gamma_hip_ivfpq_set_trained(m, coarse_centroids_.data(), pq_centroids_.data(), nullptr);
  });
  if (!rc && grp_) {
    // list -> GPU by the training set's list sizes, balanced greedily: the lists never move afterwards
    std::vector<int32_t> assign(num);
    rc = gamma_hip_assign(h_, d_, (int64_t)num, xt.data(), nlist_, coarse_centroids_.data(), assign.data(), nullptr);
    std::vector<int64_t> weight(nlist_, 0);
    for (size_t i = 0; i < num && !rc; i++)
      if (assign[i] >= 0 && assign[i] < nlist_) weight[assign[i]]++;
    if (!rc) rc = gamma_hip_group_set_owners(grp_, weight.data());
  }
  if (rc) {
    HLOG("training failed: %s (%s)", gamma_hip_strerror(rc), gamma_hip_last_error(h_));
    return -1;
  }
  is_trained_ = true;
  return 0;
}

// the first `num` vectors of the store, num by the rule of gamma_index_ivfpq.cc:280-301 (= gamma_index_ivfflat.cc:252-276)
int GammaIVFPQHIPIndex::TrainingSet(std::vector<float> &xt, size_t &num) {
  const size_t vectors_count = vector_->MetaInfo()->Size();
  if ((size_t)indexing_size_ < (size_t)nlist_) num = (size_t)nlist_ * 39;
  else if ((size_t)indexing_size_ <= (size_t)nlist_ * 256) num = (size_t)indexing_size_;
  else num = (size_t)nlist_ * 256;
  if (num > vectors_count) {
    HLOG("vector total count [%zu] less then index_size[%zu], failed!", vectors_count, num);
    return -1;
  }
  std::vector<int64_t> vids(num);
  for (size_t i = 0; i < num; i++) vids[i] = (int64_t)i;
  ScopeVectors sv;
  if (vector_->Gets(vids, sv)) return -1;
  xt.resize(num * d_);
  for (size_t i = 0; i < num; i++) memcpy(&xt[i * d_], sv.Get((int)i), sizeof(float) * d_);
  return 0;
}

int HIPParseRawDtype(const char *model, const std::string &model_parameters, int *et) {
  *et = 0;
  if (model_parameters == "") return 0;
  utils::JsonParser jp;
  if (jp.Parse(model_parameters.c_str())) return -1;
  std::string rdt;
  if (jp.GetString("raw_dtype", rdt)) return 0;
  static const char *const names[4] = {"float32", "float16", "uint8", "int8"};
  for (int i = 0; i < 4; i++)
    if (!strcasecmp(names[i], rdt.c_str())) {
      *et = i;
      return 0;
    }
  fprintf(stderr, "[%s] invalid raw_dtype = %s\n", model, rdt.c_str());
  return -1;
}

bool HIPRowsStorableI8(const HIPRawI8Ops *ops, bool is_signed, int d, const char *model, const char *what, const float *x,
                       int64_t nrows) {
  int64_t bad = -1;
  if (!ops->check(x, nrows * d, is_signed ? 1 : 0, &bad)) return true;
  fprintf(stderr, "[%s] %s refused: raw_dtype = %s stores a value only if it converts exactly, and element %d of row %lld is %g\n",
          model, what, is_signed ? "int8" : "uint8", (int)(bad % d), (long long)(bad / d), (double)x[bad]);
  return false;
}

bool GammaIVFPQHIPIndex::RowsStorable(const char *what, const float *x, int64_t nrows) {
  if (raw_sq8_ops_) {
    int64_t bad = -1;
    if (!raw_sq8_ops_->check(x, nrows * d_, &bad)) return true;
    fprintf(stderr, "[HIPIVFPQ] %s refused: raw_dtype = sq8 stores a value only if it is finite, and element %d of row %lld is %g\n",
            what, (int)(bad % d_), (long long)(bad / d_), (double)x[bad]);
    return false;
  }
  if (raw_f16_ && rawshard_) {
    // float16 rows sharded with their lists: the members' rule (a finite value that rounds to an infinite half is refused), here
    // so that a refused Add comes before the placement switches and before any member is asked
    for (int64_t i = 0; i < nrows * d_; i++) {
      const float a = std::fabs(x[i]);
      if (a >= 65520.f && a != std::numeric_limits<float>::infinity()) {
        fprintf(stderr, "[HIPIVFPQ] %s refused: raw_dtype = float16 stores a finite value only inside binary16's range, and element %d of row %lld is %g\n",
                what, (int)(i % d_), (long long)(i / d_), (double)x[i]);
        return false;
      }
    }
    return true;
  }
  return !raw_i8_ || HIPRowsStorableI8(raw_i8_ops_, raw_i8_ == 2, d_, "HIPIVFPQ", what, x, nrows);
}

bool GammaIVFPQHIPIndex::Add(int n, const uint8_t *vec) {
  // vids are consecutive from indexed_vec_count_ (gamma_index_ivfpq.cc:475-489); the raw
  // vectors are mirrored to HBM for the exact re-rank (VectorReader::Gets on the CPU path).
  // The mirror is written at explicit rows (gamma_hip_raw_write): a brute-force Search that mirrors the
  // same rows at the same time (EnsureRaw) rewrites identical bytes instead of appending them twice.
  const float *v = reinterpret_cast<const float *>(vec);
  const int64_t end = (int64_t)indexed_vec_count_ + n;
  if (!RowsStorable("add", v, n)) return false;   // before anything changes: no row, no key
  if (rawshard_) {
    // sharded rows: the group puts every row beside its keys at the owner of its list (gamma_hip_group_ivfpq_add below);
    // the first Add after training retires member 0's mirror of the untrained model
    if (ShardRows()) return false;
  } else {
    if (EnsureRaw(indexed_vec_count_)) return false;
    std::lock_guard<std::mutex> g(raw_mu_);
    if (ForAll([&](gamma_hip_index *m) { return gamma_hip_raw_write(m, indexed_vec_count_, n, v); })) return false;
    raw_uploaded_ = std::max(raw_uploaded_, end);
  }
  if (SyncVid2DocID(end)) return false;   // before AddKeys: it counts vectors of deleted DOCS (realtime_mem_data.cc:294)
  int rc = grp_ ? gamma_hip_group_ivfpq_add(grp_, n, v, indexed_vec_count_) : gamma_hip_ivfpq_add(h_, n, v, indexed_vec_count_);
  if (rc) {
    HLOG("add failed: %s (%s)", gamma_hip_strerror(rc), grp_ ? gamma_hip_group_last_error(grp_) : gamma_hip_last_error(h_));
    return false;
  }
  indexed_vec_count_ += n;
  return true;
}

int GammaIVFPQHIPIndex::Update(const std::vector<int64_t> &ids, const std::vector<const uint8_t *> &vecs) {
  // the engine drains up to 20 000 updated vids per pass (vector/vector_manager.cc:355-380): ONE encode of the batch
  // (each vector assigned as quantizer->assign(1, ..) assigns it, gamma_index_ivfpq.cc:398), the list updates in
  // order, one publish -- instead of two device round trips per vid
  const size_t n = ids.size();
  if (n == 0) return 0;
  if (vecs.size() != n) return -1;
  std::vector<float> x(n * (size_t)d_);
  for (size_t i = 0; i < n; i++) memcpy(&x[i * d_], vecs[i], sizeof(float) * d_);
  if (!RowsStorable("update", x.data(), (int64_t)n)) return -1;   // before the lists change
  int rc = grp_ ? gamma_hip_group_ivfpq_update(grp_, (int)n, ids.data(), x.data())
                : gamma_hip_ivfpq_update_batch(h_, (int)n, ids.data(), x.data());
  if (rc) {
    HLOG("update failed: %s (%s)", gamma_hip_strerror(rc), grp_ ? gamma_hip_group_last_error(grp_) : gamma_hip_last_error(h_));
    return -1;
  }
  {
    std::lock_guard<std::mutex> g(raw_mu_);   // rows the mirror has not reached yet are skipped: EnsureRaw brings them
    if (rawshard_) {
      // sharded rows: the group's Update has rewritten or moved them with their vectors; before that only member 0 mirrors
      if (!rows_sharded_ && gamma_hip_raw_update_batch(h_, (int64_t)n, ids.data(), x.data())) return -1;
    } else if (ForAll([&](gamma_hip_index *m) { return gamma_hip_raw_update_batch(m, (int64_t)n, ids.data(), x.data()); })) {
      return -1;
    }
  }
  if (grp_) gamma_hip_group_ivfpq_compact_if_need(grp_);
  else gamma_hip_ivfpq_compact_if_need(h_);   // gamma_index_ivfpq.cc:420
  if (model_param_ && model_param_->device_filters) {
    // the engine updated these docs (table first, then this model): the device mirror of their scalar fields follows
    std::vector<int64_t> docs(ids);
    RawVector *rv = dynamic_cast<RawVector *>(vector_);
    if (rv && rv->VidMgr() && rv->VidMgr()->MultiVids())
      for (size_t i = 0; i < docs.size(); i++) docs[i] = rv->VidMgr()->VID2DocID((int)ids[i]);
    if (columns_.Refresh(h_, docs)) return -1;
  }
  return 0;
}

int GammaIVFPQHIPIndex::Delete(const std::vector<int64_t> &ids) {
  // the engine sets the doc bit in its BitmapManager (search/gamma_engine.cc:810-812); the
  // device keeps a mirror of that bitmap, fed from here (vid == docid for single-vector docs)
  if (ids.empty()) return 0;
  // the bitmap is on DOC ids (VIDMgr::VID2DocID; the identity for single-vector documents)
  std::vector<int64_t> docs(ids);
  RawVector *rv = dynamic_cast<RawVector *>(vector_);
  if (rv && rv->VidMgr() && rv->VidMgr()->MultiVids())
    for (size_t i = 0; i < docs.size(); i++) docs[i] = rv->VidMgr()->VID2DocID((int)ids[i]);
  if (ForAll([&](gamma_hip_index *m) { return gamma_hip_bitmap_set(m, docs.data(), (int64_t)docs.size(), 1); })) return -1;
  if (grp_) return gamma_hip_group_ivfpq_delete(grp_, ids.data(), (int)ids.size()) ? -1 : 0;
  return gamma_hip_ivfpq_delete(h_, ids.data(), (int)ids.size()) ? -1 : 0;
}

int GammaIVFPQHIPIndex::Search(RetrievalContext *retrieval_context, int n, const uint8_t *x, int k,
                               float *distances, int64_t *ids) {
  HIPIVFPQRetrievalParameters *rp = dynamic_cast<HIPIVFPQRetrievalParameters *>(retrieval_context->RetrievalParams());
  HIPIVFPQRetrievalParameters defaults;
  if (rp == nullptr) rp = &defaults;
  GammaSearchCondition *cond = dynamic_cast<GammaSearchCondition *>(retrieval_context);
  gamma_hip_search_params p;
  memset(&p, 0, sizeof(p));
  p.metric = rp->GetDistanceComputeType() == DistanceComputeType::INNER_PRODUCT ? GAMMA_HIP_METRIC_IP
                                                                                : GAMMA_HIP_METRIC_L2;
  p.recall_num = rp->RecallNum();
  p.has_rank = cond ? (cond->has_rank ? 1 : 0) : 1;
  p.min_score = cond ? cond->min_score : std::numeric_limits<float>::min();
  p.max_score = cond ? cond->max_score : std::numeric_limits<float>::max();
  p.coarse_mode = -1;
  p.exact_ties = rp->ExactTies();
  std::vector<gamma_hip_range_filter> rf;
  std::vector<gamma_hip_field_filter> ff;
  std::vector<gamma_hip_term_filter> tf;
  // scalar filters: on the device against mirrored columns when asked for and possible, else the request's
  // flattened docid bitmaps as the CPU models take them
  if (!(model_param_ && model_param_->device_filters &&
        columns_.Prepare(h_, cond, DocCountOf(this, (int64_t)vector_->MetaInfo()->Size()), p, ff, tf)))
    FillRangeFilters(cond, p, rf);
  const float *xq = reinterpret_cast<const float *>(x);
  int rc;
  if (((cond && cond->brute_force_search) || !is_trained_) && raw_f16_) {
    // the flat search reads fp32 rows, the device holds rounded ones: refused, never an answer over other rows
    HLOG("brute_force_search (and the search of an untrained model) is not available with raw_dtype = float16");
    return -3;
  }
  if (((cond && cond->brute_force_search) || !is_trained_) && raw_i8_) {
    HLOG("brute_force_search (and the search of an untrained model) is not available with raw_dtype = %s",
         raw_i8_ == 2 ? "int8" : "uint8");
    return -3;
  }
  if (((cond && cond->brute_force_search) || !is_trained_) && raw_sq8_ops_) {
    HLOG("brute_force_search (and the search of an untrained model) is not available with raw_dtype = sq8");
    return -3;
  }
  if (((cond && cond->brute_force_search) || !is_trained_) && rawshard_) {
    // sharded rows: member 0 mirrors the store until the first Add after training; the mirror cannot go away under the
    // flat search (raw_mu_ through the call).  Afterwards no device holds every row: refused, never a wrong answer.
    std::lock_guard<std::mutex> g(raw_mu_);
    if (rows_sharded_) {
      HLOG("brute_force_search is not available once the raw vectors are sharded (raw_placement = sharded)");
      return -3;
    }
    if (EnsureRawLocked((int64_t)vector_->MetaInfo()->Size())) return -1;
    rc = gamma_hip_flat_search(h_, &p, n, xq, k, distances, ids);
  } else if ((cond && cond->brute_force_search) || !is_trained_) {
    if (EnsureRaw((int64_t)vector_->MetaInfo()->Size())) return -1;
    rc = gamma_hip_flat_search(h_, &p, n, xq, k, distances, ids);   // gamma_index_ivfpq.cc:529-537
  } else {
    // nprobe rule of gamma_index_ivfpq.cc:539-545
    p.nprobe = (rp->Nprobe() > 0 && rp->Nprobe() <= nlist_) ? rp->Nprobe() : nprobe_;
    rc = grp_ ? gamma_hip_group_ivfpq_search(grp_, &p, n, xq, k, distances, ids)
              : gamma_hip_ivfpq_search(h_, &p, n, xq, k, distances, ids);
  }
  PerfLabels(cond);
  if (rc) {
    HLOG("search failed: %s (%s)", gamma_hip_strerror(rc), grp_ ? gamma_hip_group_last_error(grp_) : gamma_hip_last_error(h_));
    return rc;
  }
  WarnTiesNotHonoured(h_, grp_, &ties_said_);
  WarnBlasCorners(h_, grp_, &blas_said_);
  return 0;
}

// A search beyond the exact-ties mode's range (nprobe > 1024, a flat search for k = 4096) that merely inherited the model's
// default ran with the (distance, position) order inside ties: said once per new occurrence count of THIS model (the
// high-water mark is a member of the index object; a group's count is the sum over its members), never silently
// (gamma_hip_ties_not_honoured; a request that sets "exact_ties": 1 itself fails instead).  The same line reports repack
// read-backs that differed from their source (gamma_hip_ivfpq_repack_verify_stats).
void WarnTiesNotHonoured(gamma_hip_index *h, gamma_hip_group *grp, std::atomic<int64_t> *said) {
  int64_t n = 0, bad_repacks = 0;
  const int members = grp ? gamma_hip_group_size(grp) : 1;
  for (int i = 0; i < members; i++) {
    gamma_hip_index *m = grp ? gamma_hip_group_member(grp, i) : h;
    int64_t c = 0, rv[2] = {0, 0};
    if (m && !gamma_hip_ties_not_honoured(m, &c, 0)) n += c;
    if (m && !gamma_hip_ivfpq_repack_verify_stats(m, rv)) bad_repacks += rv[1];
  }
  const int64_t mark = n + (bad_repacks << 40);
  if (mark <= 0 || !said) return;
  int64_t prev = said->load();
  if (mark > prev && said->compare_exchange_strong(prev, mark)) {
    if (n > 0)
      HLOG("%lld search call(s) ran without the reference's heap order inside exact ties: shape beyond the mode's range "
           "(nprobe > 1024 or flat k = 4096)", (long long)n);
    if (bad_repacks > 0)
      HLOG("%lld list-arena repack(s) did not read back as written: the previous arena was kept and the move repeated into "
           "ordinary allocations", (long long)bad_repacks);
  }
}

// Calls whose GEMM-form coarse distances fell into a shape for which the library's sgemm_ kernel is not restated
// (gamma_hip_blas_form_not_restated: ulp-level differences in a few coarse distances): logged when the count first
// becomes non-zero and at every doubling -- an Add stream of odd batch sizes would otherwise fill the log.
void WarnBlasCorners(gamma_hip_index *h, gamma_hip_group *grp, std::atomic<int64_t> *said) {
  int64_t n = 0;
  const int members = grp ? gamma_hip_group_size(grp) : 1;
  for (int i = 0; i < members; i++) {
    gamma_hip_index *m = grp ? gamma_hip_group_member(grp, i) : h;
    int64_t c = 0;
    if (m && !gamma_hip_blas_form_not_restated(m, &c, 0)) n += c;
  }
  if (n <= 0 || !said) return;
  int64_t prev = said->load();
  if (n >= 2 * prev && n > prev && said->compare_exchange_strong(prev, n))
    HLOG("%lld call(s) computed coarse distances in a GEMM shape whose MKL kernel is not restated (K > 768, K = 384 with a "
         "9..512-row remainder, remainder blocks of 1..7 rows): a few coarse distances may differ from faiss's by an ulp",
         (long long)n);
}

// PerfTool (index/retrieval_model.h:23-50; printed by the engine at online_log_level=debug): one label for the device
// call, and with "perf_stages": 1 the device time of every stage of the handle's searches since the last label
// (HIP events, gamma_hip_profile_get; concurrent searches share the counters)
void GammaIVFPQHIPIndex::PerfLabels(GammaSearchCondition *cond) {
  if (!cond || !cond->perf_tool_) return;
  cond->GetPerfTool().Perf("hip search");
  if (!(model_param_ && model_param_->perf_stages) || grp_) return;
  static const char *names[] = {"coarse", "tables", "scan", "select", "rerank", "flat"};
  std::lock_guard<std::mutex> g(perf_mu_);
  for (int st = 0; st < GAMMA_HIP_NUM_STAGES; st++) {
    double ms = 0;
    int64_t launches = 0;
    if (gamma_hip_profile_get(h_, st, &ms, &launches)) continue;
    if (ms > perf_ms_[st]) cond->GetPerfTool().perf_ss << "hip " << names[st] << " [" << ms - perf_ms_[st] << "]ms ";
    perf_ms_[st] = ms;
  }
}

// mirror vids [raw_uploaded_, upto) of the engine's vector store into HBM.  Called from Search (any number of
// client threads: brute force before training), from Add (the indexing thread) and from Load: raw_mu_ makes
// "read the watermark, copy, advance it" one step, and the rows go to their own positions.
int GammaIVFPQHIPIndex::EnsureRaw(int64_t upto) {
  std::lock_guard<std::mutex> g(raw_mu_);
  return EnsureRawLocked(upto);
}

int GammaIVFPQHIPIndex::EnsureRawLocked(int64_t upto) {
  if (rows_sharded_) return 0;   // the group holds the rows
  const int64_t step = 65536;
  for (int64_t i0 = raw_uploaded_; i0 < upto; i0 += step) {
    const int64_t nb = std::min(step, upto - i0);
    std::vector<int64_t> vids(nb);
    for (int64_t i = 0; i < nb; i++) vids[i] = i0 + i;
    ScopeVectors sv;
    if (vector_->Gets(vids, sv)) return -1;
    std::vector<float> buf((size_t)nb * d_);
    for (int64_t i = 0; i < nb; i++) memcpy(&buf[(size_t)i * d_], sv.Get((int)i), sizeof(float) * d_);
    // ("raw_placement": "sharded": the mirror of the untrained model lives on member 0 alone -- brute force runs there)
    if (rawshard_ ? gamma_hip_raw_write(h_, i0, nb, buf.data())
                  : ForAll([&](gamma_hip_index *m) { return gamma_hip_raw_write(m, i0, nb, buf.data()); }))
      return -1;
    raw_uploaded_ = i0 + nb;
  }
  return 0;
}

// "raw_placement": "sharded", once: member 0's mirror by vid is cleared and the group switches to sharded rows
int GammaIVFPQHIPIndex::ShardRows() {
  std::lock_guard<std::mutex> g(raw_mu_);
  if (rows_sharded_) return 0;
  int rc = rawshard_->raw_clear(h_);
  if (!rc) rc = rawshard_->set_raw_placement(grp_, 1);
  if (rc) {
    HLOG("cannot shard the raw vectors: %s (%s)", gamma_hip_strerror(rc), gamma_hip_group_last_error(grp_));
    return -1;
  }
  raw_uploaded_ = 0;
  rows_sharded_ = true;
  return 0;
}

// after a Load: every owner gets the rows of its lists from the engine's vector store, in bounded batches (vids nobody
// lists -- superseded by an Update before the dump -- are skipped by the group)
int GammaIVFPQHIPIndex::PutRowsFromStore(int64_t upto) {
  const int64_t step = 65536;
  for (int64_t i0 = 0; i0 < upto; i0 += step) {
    const int64_t nb = std::min(step, upto - i0);
    std::vector<int64_t> vids(nb);
    for (int64_t i = 0; i < nb; i++) vids[i] = i0 + i;
    ScopeVectors sv;
    if (vector_->Gets(vids, sv)) return -1;
    std::vector<float> buf((size_t)nb * d_);
    for (int64_t i = 0; i < nb; i++) memcpy(&buf[(size_t)i * d_], sv.Get((int)i), sizeof(float) * d_);
    int64_t skipped = 0;
    const int rc = rawshard_->group_raw_put(grp_, nb, vids.data(), buf.data(), &skipped);
    if (rc) {
      HLOG("cannot restore the raw vectors: %s (%s)", gamma_hip_strerror(rc), gamma_hip_group_last_error(grp_));
      return -1;
    }
  }
  return 0;
}

// the engine's delete bitmap -> the device mirror (after a restart the engine has loaded its bitmap file
// before it calls Load on the models, util/bitmap_manager.cc:96-161; vector_ is a RawVector, raw_vector.h:171)
// multi-vector documents: the device tests the delete bitmap and every filter on the DOC id of a scanned vector
// (include/gamma_hip.h gamma_hip_vid2docid_append); the mapping is the engine's VIDMgr
int GammaIVFPQHIPIndex::SyncVid2DocID(int64_t upto) {
  RawVector *rv = dynamic_cast<RawVector *>(vector_);
  if (!rv || !rv->VidMgr() || !rv->VidMgr()->MultiVids()) return 0;
  const int64_t have = gamma_hip_vid2docid_count(h_);
  if (have < 0) return -1;
  if (upto <= have) return 0;
  std::vector<int32_t> m((size_t)(upto - have));
  for (int64_t v = have; v < upto; v++) m[(size_t)(v - have)] = rv->VidMgr()->VID2DocID((int)v);
  return ForAll([&](gamma_hip_index *mm) { return gamma_hip_vid2docid_append(mm, (int64_t)m.size(), m.data()); });
}

int GammaIVFPQHIPIndex::UploadEngineBitmap() {
  RawVector *rv = dynamic_cast<RawVector *>(vector_);
  if (!rv || !rv->Bitmap() || rv->Bitmap()->BitSize() == 0) return 0;
  return ForAll([&](gamma_hip_index *m) {
    return gamma_hip_bitmap_upload(m, reinterpret_cast<const uint8_t *>(rv->Bitmap()->Bitmap()), (int64_t)rv->Bitmap()->BitSize());
  });
}

int GammaIVFPQHIPIndex::SetTrained(const float *coarse, const float *pq) {
  coarse_centroids_.assign(coarse, coarse + (size_t)nlist_ * d_);
  pq_centroids_.assign(pq, pq + (size_t)M_ * Ksub() * (d_ / M_));
  if (ForAll([&](gamma_hip_index *m) {
        return gamma_hip_ivfpq_set_trained(m, coarse_centroids_.data(), pq_centroids_.data(), nullptr);
      }))
    return -1;
  // several GPUs: no list sizes to balance yet -- lists are dealt round robin (Indexing balances by the training
  // set's assignment, Load by the dumped sizes)
  if (grp_ && gamma_hip_group_owner(grp_, 0) < 0 && gamma_hip_group_set_owners(grp_, nullptr)) return -1;
  is_trained_ = true;
  return 0;
}

long GammaIVFPQHIPIndex::GetTotalMemBytes() {
  if (grp_) return (long)gamma_hip_group_total_mem_bytes(grp_);
  return h_ ? (long)gamma_hip_total_mem_bytes(h_) : 0;
}

// Dump / Load in the reference's own file format (gamma_index_ivfpq.cc:958-1048): an index dumped by
// the CPU "IVFPQ" model loads here and the other way round (iwpq_io.h for the record layout).
int GammaIVFPQHIPIndex::Dump(const std::string &dir) {
  if (!is_trained_) {
    HLOG("index is not trained, skip dumping");
    return 0;
  }
  const std::string index_dir = dir + "/" + vector_->MetaInfo()->AbsoluteName();
  if (mkdir(index_dir.c_str(), 0755) && errno != EEXIST) {
    HLOG("mkdir error, index dir=%s", index_dir.c_str());
    return -1;
  }
  IwPQFile f;
  f.d = d_;
  f.ntotal = 0;   // GammaIVFPQIndex never advances faiss's ntotal; its dumps carry 0
  f.metric = metric_type_ == DistanceComputeType::INNER_PRODUCT ? 0 : 1;
  f.nlist = (size_t)nlist_;
  f.nprobe = (size_t)nprobe_;
  f.coarse = coarse_centroids_;
  f.by_residual = true;
  f.code_size = CodeSize();
  f.M = (size_t)M_;
  f.nbits = (size_t)nbits_;
  f.pq = pq_centroids_;
  if (opq_) f.opq = opq_A_;   // the "LTra" record between the product quantizer and the lists (gamma_index_ivfpq.cc:979-984)
  f.sizes.resize(nlist_);
  f.codes.resize(nlist_);
  f.ids.resize(nlist_);
  for (int l = 0; l < nlist_; l++) {
    const int64_t len = grp_ ? gamma_hip_group_ivfpq_list_size(grp_, l) : gamma_hip_ivfpq_list_size(h_, l);
    if (len < 0) return -1;
    f.sizes[l] = (size_t)len;
    if (len == 0) continue;
    f.ids[l].resize(len);
    f.codes[l].resize((size_t)len * CodeSize());
    if (grp_ ? gamma_hip_group_ivfpq_get_list(grp_, l, f.ids[l].data(), f.codes[l].data())
             : gamma_hip_ivfpq_get_list(h_, l, f.ids[l].data(), f.codes[l].data()))
      return -1;
  }
  if (WriteIwPQ(index_dir + "/ivfpq.index", f)) {
    HLOG("write error, index dir=%s", index_dir.c_str());
    return -1;
  }
  if (raw_sq8_ops_ && DumpSq8Ranges(index_dir)) return -1;   // a side file: ivfpq.index stays what the reference writes
  return 0;
}

// raw_sq8.ranges: magic "SQ8R", int32 d, d floats vmin, d floats vmax
namespace {
const char kSq8RangesMagic[4] = {'S', 'Q', '8', 'R'};
}
int GammaIVFPQHIPIndex::DumpSq8Ranges(const std::string &index_dir) {
  std::vector<float> r((size_t)d_ * 2);
  if (raw_sq8_ops_->get_ranges(h_, r.data(), r.data() + d_)) {
    HLOG("cannot read the sq8 ranges: %s", gamma_hip_last_error(h_));
    return -1;
  }
  const std::string path = index_dir + "/raw_sq8.ranges";
  FILE *fp = fopen(path.c_str(), "wb");
  const int32_t d32 = d_;
  const bool ok = fp && fwrite(kSq8RangesMagic, 1, 4, fp) == 4 && fwrite(&d32, sizeof(d32), 1, fp) == 1 &&
                  fwrite(r.data(), sizeof(float), r.size(), fp) == r.size();
  if ((fp && fclose(fp)) || !ok) {
    HLOG("write error, %s", path.c_str());
    return -1;
  }
  return 0;
}

int GammaIVFPQHIPIndex::Sq8Ranges(float *vmin, float *vmax) {
  if (!raw_sq8_ops_) return -1;
  return raw_sq8_ops_->get_ranges(h_, vmin, vmax) ? 0 : 1;
}

int GammaIVFPQHIPIndex::LoadSq8Ranges(const std::string &index_dir) {
  const std::string path = index_dir + "/raw_sq8.ranges";
  FILE *fp = fopen(path.c_str(), "rb");
  if (!fp) {
    HLOG("raw_dtype = sq8 needs %s beside the index file (the ranges the rows were encoded with), and it is missing", path.c_str());
    return -1;
  }
  char magic[4] = {0, 0, 0, 0};
  int32_t d32 = 0;
  std::vector<float> r((size_t)d_ * 2);
  const bool head = fread(magic, 1, 4, fp) == 4 && fread(&d32, sizeof(d32), 1, fp) == 1;
  const bool ok = head && !memcmp(magic, kSq8RangesMagic, 4) && d32 == d_ && fread(r.data(), sizeof(float), r.size(), fp) == r.size();
  fclose(fp);
  if (!ok) {
    HLOG("%s is not the sq8 ranges of a %d-dimensional model (bad magic, another dimension or a short file)", path.c_str(), d_);
    return -1;
  }
  if (raw_sq8_ops_->set_ranges(h_, r.data(), r.data() + d_)) {
    HLOG("cannot set the sq8 ranges: %s", gamma_hip_last_error(h_));
    return -1;
  }
  return 0;
}

int GammaIVFPQHIPIndex::Load(const std::string &dir) {
  const std::string path = dir + "/" + vector_->MetaInfo()->AbsoluteName() + "/ivfpq.index";
  FILE *probe = fopen(path.c_str(), "rb");
  if (!probe) {
    HLOG("%s isn't existed, skip loading", path.c_str());
    return 0;   // it should train again after load
  }
  fclose(probe);
  IwPQFile f;
  const int rc = ReadIwPQ(path, &f);
  if (rc) {
    HLOG("cannot read %s (%d)", path.c_str(), rc);
    return -1;
  }
  if (f.d != d_ || (int)f.nlist != nlist_ || (int)f.M != M_ || (int)f.nbits != nbits_ || f.code_size != CodeSize() ||
      !f.by_residual || f.pq.size() != (size_t)M_ * Ksub() * (d_ / M_)) {
    HLOG("index file does not match the table's retrieval_param");
    return -1;
  }
  if ((opq_ != nullptr) != !f.opq.empty()) {
    HLOG("index file %s an opq record, the table's retrieval_param %s opq", f.opq.empty() ? "has no" : "has",
         opq_ ? "names" : "does not name");
    return -1;
  }
  // "raw_dtype": "sq8": the ranges come back before anything of the model changes and before the mirror is re-encoded below
  if (raw_sq8_ops_ && LoadSq8Ranges(dir + "/" + vector_->MetaInfo()->AbsoluteName())) return -1;
  if (opq_) {   // read_opq (gamma_index_ivfpq.cc:1017-1019): on the handle before the lists are filled
    if (opq_->set(h_, f.opq.data())) {
      HLOG("cannot set the opq matrix: %s", gamma_hip_last_error(h_));
      return -1;
    }
    opq_A_ = f.opq;
  }
  if (grp_) {   // several GPUs: list -> GPU balanced by the dumped list sizes, before the lists come back
    std::vector<int64_t> weight(nlist_);
    for (int l = 0; l < nlist_; l++) weight[l] = (int64_t)f.sizes[l];
    if (gamma_hip_group_set_owners(grp_, weight.data())) return -1;
  }
  if (SetTrained(f.coarse.data(), f.pq.data())) return -1;   // T2 is recomputed, as in the reference
  // deletes that happened before the restart: the bitmap must be in place BEFORE the lists come back, so that
  // AddKeys counts the deleted entries per list as the reference does (realtime_mem_data.cc:293-296)
  if (UploadEngineBitmap()) return -1;
  if (SyncVid2DocID((int64_t)vector_->MetaInfo()->Size())) return -1;
  metric_type_ = f.metric == 0 ? DistanceComputeType::INNER_PRODUCT : DistanceComputeType::L2;
  int64_t count = 0;
  for (int l = 0; l < nlist_; l++) {
    const size_t n = f.sizes[l];
    if (n == 0) continue;
    if (grp_ ? gamma_hip_group_ivfpq_add_keys(grp_, l, (int)n, f.ids[l].data(), f.codes[l].data())
             : gamma_hip_ivfpq_add_keys(h_, l, (int)n, f.ids[l].data(), f.codes[l].data()))
      return -1;
    for (size_t i = 0; i < n; i++)
      if (f.ids[l][i] >= 0) count++;   // bit 63 = superseded by an Update (gamma_index_io.cc:186-189)
  }
  indexed_vec_count_ = (int)count;
  // raw vectors for the re-rank come back from the engine's vector store
  const int64_t rows = std::min<int64_t>(indexed_vec_count_, (int64_t)vector_->MetaInfo()->Size());
  if (rawshard_) {
    if (ShardRows() || PutRowsFromStore(rows)) return -1;
  } else if (EnsureRaw(rows)) {
    return -1;
  }
  return indexed_vec_count_;
}


// ------------------------------------------------------------------------------------------------------------
// HIPIVFFLAT (gamma_index_ivfflat.{h,cc})
// ------------------------------------------------------------------------------------------------------------
REGISTER_MODEL(HIPIVFFLAT, GammaIVFFlatHIPIndex);

namespace {
HIPIVFFlatRowsFn &IVFFlatRows() {
  static HIPIVFFlatRowsFn fn = nullptr;
  return fn;
}
}  // namespace
int RegisterHIPIVFFlatRows(HIPIVFFlatRowsFn fn) {
  IVFFlatRows() = fn;
  return 0;
}
HIPIVFFlatRowsFn FindHIPIVFFlatRows() { return IVFFlatRows(); }

namespace {
HIPIVFFlatSq8RowsFn &IVFFlatSq8Rows() {
  static HIPIVFFlatSq8RowsFn fn = nullptr;
  return fn;
}
}  // namespace
int RegisterHIPIVFFlatSq8Rows(HIPIVFFlatSq8RowsFn fn) {
  IVFFlatSq8Rows() = fn;
  return 0;
}
HIPIVFFlatSq8RowsFn FindHIPIVFFlatSq8Rows() { return IVFFlatSq8Rows(); }

namespace {
HIPIVFFlatGroupSearchFn &IVFFlatGroupSearch() {
  static HIPIVFFlatGroupSearchFn fn = nullptr;
  return fn;
}
}  // namespace
int RegisterHIPIVFFlatGroup(HIPIVFFlatGroupSearchFn fn) {
  IVFFlatGroupSearch() = fn;
  return 0;
}
HIPIVFFlatGroupSearchFn FindHIPIVFFlatGroup() { return IVFFlatGroupSearch(); }

namespace {
HIPIVFFlatGroupRowsFn &IVFFlatGroupRows() {
  static HIPIVFFlatGroupRowsFn fn = nullptr;
  return fn;
}
}  // namespace
int RegisterHIPIVFFlatGroupRows(HIPIVFFlatGroupRowsFn fn) {
  IVFFlatGroupRows() = fn;
  return 0;
}
HIPIVFFlatGroupRowsFn FindHIPIVFFlatGroupRows() { return IVFFlatGroupRows(); }

int GammaIVFFlatHIPIndex::DeviceKeys(const std::string &model_parameters, int et, HIPIVFPQModelParams &pa, bool *several,
                                     bool *members_narrow) {
  *several = *members_narrow = false;
  // several devices ("devices": "0,1,..", HIPIVFPQ's keys and parser): the in-process group, where the build carries its IVFFLAT
  // search (gamma_index_ivfflat_group_hip.cc); without it the keys stay unread and the model opens one handle, as it always did
  if (!FindHIPIVFFlatGroup()) return 0;
  utils::JsonParser jp;
  if (model_parameters != "" && jp.Parse(model_parameters.c_str())) return -1;
  if (ParseDeviceKeys(jp, pa)) return -1;
  *several = pa.devices.size() > 1;
  // "group_rows": "raw_dtype" (gamma_index_ivfflat_group_rows_hip.cc): the members hold their rows in a narrow raw_dtype
  int narrow = 0;
  const HIPIVFFlatGroupRowsFn group_rows = FindHIPIVFFlatGroupRows();
  if (group_rows && group_rows(model_parameters, et, pa.devices.size(), pa.device_filters, &narrow)) return -1;
  *members_narrow = narrow != 0;
  if (*several && et != 0 && !narrow) {
    HLOG("HIPIVFFLAT: raw_dtype other than float32 with several devices is not supported (the group's members hold fp32 rows)");
    return -1;
  }
  if (*several && pa.device_filters) {
    HLOG("HIPIVFFLAT: device_filters with several devices is not supported (the columns live on one handle)");
    return -1;
  }
  if (pa.raw_sharded) {
    const HIPRawShardOps *rawshard = FindHIPRawShard();
    if (!*several || pa.replicate || !rawshard) {
      HLOG("HIPIVFFLAT: raw_placement = sharded needs several devices and placement = shard%s",
           rawshard ? "" : " (and this build of the plugin carries no sharded raw rows)");
      return -1;
    }
  }
  return 0;
}

void GammaIVFFlatHIPIndex::CheckGroupKeys(const std::string &model_parameters, int *out) {
  out[0] = out[1] = out[2] = 0;
  HIPIVFPQModelParams pa;
  utils::JsonParser jp;
  int v = 0, et = 0;
  if (model_parameters != "" && jp.Parse(model_parameters.c_str())) {
    out[0] = -1;
    return;
  }
  if (!jp.GetInt("device_filters", v)) pa.device_filters = v != 0;
  bool several = false, members_narrow = false;
  out[0] = ParseRawDtype(model_parameters, &et) ? -1 : DeviceKeys(model_parameters, et, pa, &several, &members_narrow);
  out[1] = !out[0] && several;
  out[2] = !out[0] && members_narrow;
}

int GammaIVFFlatHIPIndex::ParseRawDtype(const std::string &model_parameters, int *et) {
  *et = 0;
  utils::JsonParser jp;
  const bool parsed = model_parameters != "" && !jp.Parse(model_parameters.c_str());
  std::string rdt;
  const bool sq8 = parsed && !jp.GetString("raw_dtype", rdt) && !strcasecmp("sq8", rdt.c_str());
  const bool has_key = parsed && jp.Contains("sq8_ranges");
  if (!(sq8 && has_key)) {
    // every other case: the answer shared with HIPFLAT, which rejects "sq8" -- alone and beside sq8_min / sq8_max, as before
    if (HIPParseRawDtype("HIPIVFFLAT", model_parameters, et)) return -1;
    if (has_key) {
      HLOG("HIPIVFFLAT: sq8_ranges comes with \"raw_dtype\": \"sq8\" only");
      *et = 0;
      return -1;
    }
    return 0;
  }
  std::string rng;
  if (jp.GetString("sq8_ranges", rng) || strcasecmp("trained", rng.c_str())) {
    HLOG("HIPIVFFLAT: raw_dtype = sq8 needs \"sq8_ranges\": \"trained\" (per-dimension ranges learned by Indexing), the one value defined");
    return -1;
  }
  if (jp.Contains("sq8_min") || jp.Contains("sq8_max")) {
    HLOG("HIPIVFFLAT: raw_dtype = sq8 takes no sq8_min / sq8_max: its ranges are trained");
    return -1;
  }
  *et = 4;
  return 0;
}

int GammaIVFFlatHIPIndex::Init(const std::string &model_parameters, int indexing_size) {
  indexing_size_ = indexing_size;
  model_param_ = new HIPIVFPQModelParams();   // ncentroids / nprobe / metric_type / bucket sizes / device_filters
  HIPIVFPQModelParams &pa = *model_param_;
  // IVFFlatModelParams::Parse (gamma_index_ivfflat.cc:41-101): ncentroids default 2048, nprobe 80, metric InnerProduct
  utils::JsonParser jp;
  if (model_parameters != "" && jp.Parse(model_parameters.c_str())) return -1;
  int v = 0;
  if (jp.Contains("ncentroids")) {
    if (jp.GetInt("ncentroids", v)) return -1;
    if (v > 0) pa.ncentroids = v;
    else if (v != -1) return -1;
  }
  if (!jp.GetInt("nprobe", v)) {
    if (v < -1) return -1;
    if (v > 0) pa.nprobe = v;
    if (pa.nprobe > pa.ncentroids) return -1;
  }
  std::string mt;
  if (!jp.GetString("metric_type", mt)) {
    if (strcasecmp("L2", mt.c_str()) && strcasecmp("InnerProduct", mt.c_str())) return -1;
    pa.metric_type = !strcasecmp("L2", mt.c_str()) ? DistanceComputeType::L2 : DistanceComputeType::INNER_PRODUCT;
  }
  if (!jp.GetInt("device_filters", v)) pa.device_filters = v != 0;
  if (!jp.GetInt("exact_ties", v)) pa.exact_ties = v != 0;
  if (!jp.GetInt("bucket_init_size", v) && v > 0) pa.bucket_init_size = v;
  if (!jp.GetInt("bucket_max_size", v) && v > 0) pa.bucket_max_size = v;
  int et = 0;
  if (ParseRawDtype(model_parameters, &et)) return -1;
  // a narrow store needs its initialiser and the handle's switch; a build without one of them rejects the value
  const bool narrow = et >= 1 && et <= 3;
  const HIPIVFFlatRowsFn ivfflat_rows = narrow ? FindHIPIVFFlatRows() : nullptr;
  const HIPRawInitFn init_f16 = et == 1 ? FindHIPRawInitF16() : nullptr;
  raw_i8_ops_ = et == 2 || et == 3 ? FindHIPRawI8() : nullptr;
  if (narrow && (!ivfflat_rows || (et == 1 ? !init_f16 : !raw_i8_ops_))) {
    HLOG("HIPIVFFLAT: raw_dtype: this build of the plugin has no IVFFLAT search over float16 / uint8 / int8 rows");
    return -1;
  }
  // (sq8: the store's entries that HIPIVFPQ's sq8 store registered, and the IVFFLAT search's switch for it)
  const HIPIVFFlatSq8RowsFn ivfflat_sq8_rows = et == 4 ? FindHIPIVFFlatSq8Rows() : nullptr;
  raw_sq8_ops_ = et == 4 ? FindHIPRawSq8() : nullptr;
  if (et == 4 && (!ivfflat_sq8_rows || !raw_sq8_ops_)) {
    HLOG("HIPIVFFLAT: raw_dtype: this build of the plugin has no IVFFLAT search over sq8 rows");
    return -1;
  }
  raw_f16_ = et == 1;
  raw_i8_ = narrow && et >= 2 ? et - 1 : 0;
  // several devices: the in-process group (DeviceKeys: what the keys ask, decided before a device is opened)
  group_search_ = FindHIPIVFFlatGroup();
  bool several = false, members_narrow = false;
  if (DeviceKeys(model_parameters, et, pa, &several, &members_narrow)) return -1;
  rawshard_ = group_search_ && pa.raw_sharded ? FindHIPRawShard() : nullptr;
  if (members_narrow && rawshard_ && !rawshard_->narrow_rows) {
    HLOG("HIPIVFFLAT: group_rows = raw_dtype with raw_placement = sharded: this build of the plugin has no narrow rows sharded with their lists");
    rawshard_ = nullptr;
    return -1;
  }
  if (!vector_) {
    HLOG("vector_ must be set before Init");
    return -1;
  }
  d_ = vector_->MetaInfo()->Dimension();
  nlist_ = pa.ncentroids;
  M_ = 1;   // one dummy code byte per list entry (include/gamma_hip.h, IVFFLAT)
  metric_type_ = pa.metric_type;
  nprobe_ = pa.nprobe;
  int rc;
  if (several) {
    // a group of handles, lists sharded by owner or replicated; h_ is member 0.  fp32 rows on every member, or -- "group_rows":
    // "raw_dtype" -- rows of raw_dtype: the typed store, the IVFFLAT search's switch for it and, where the rows are sharded with
    // their lists, the sparse store's; the group keeps taking fp32 vectors and the members convert
    if (OpenDevices(pa.devices, pa.replicate)) return -1;
    rc = ForAll([&](gamma_hip_index *m) {
      int r = gamma_hip_ivfflat_init(m, d_, nlist_, metric_type_ == DistanceComputeType::L2 ? GAMMA_HIP_METRIC_L2 : GAMMA_HIP_METRIC_IP,
                                     pa.bucket_init_size, pa.bucket_max_size);
      if (!r) r = !members_narrow ? gamma_hip_raw_init(m, d_) : et == 1 ? init_f16(m, d_) : raw_i8_ops_->init(m, d_, et == 3);
      if (!r && members_narrow) r = ivfflat_rows(m, 1);
      if (!r && members_narrow && rawshard_) r = rawshard_->narrow_rows(m, 1);
      if (!r) r = gamma_hip_set_exact_ties(m, pa.exact_ties ? 1 : 0);
      return r;
    });
    if (!rc && members_narrow) {
      // brute_force_search and the search of an untrained model: member 0's flat search over its narrow mirror, where the build has it
      const HIPFlatRowsFn flat_rows = FindHIPFlatRows();
      narrow_brute_ = flat_rows != nullptr;
      if (flat_rows) rc = flat_rows(h_, 1);
    }
    if (rc) {
      HLOG("device init failed: %s (%s)", gamma_hip_strerror(rc), gamma_hip_last_error(h_));
      return -1;
    }
    return 0;
  }
  const char *dev = getenv("GAMMA_HIP_DEVICE");
  rc = gamma_hip_create(dev ? atoi(dev) : 0, &h_);
  if (rc) return -1;
  members_.assign(1, h_);   // one GPU
  rc = gamma_hip_ivfflat_init(h_, d_, nlist_, metric_type_ == DistanceComputeType::L2 ? GAMMA_HIP_METRIC_L2 : GAMMA_HIP_METRIC_IP,
                              pa.bucket_init_size, pa.bucket_max_size);
  if (!rc) rc = !et ? gamma_hip_raw_init(h_, d_) : et == 1 ? init_f16(h_, d_) : et == 4 ? raw_sq8_ops_->init(h_, d_)
                                                                                         : raw_i8_ops_->init(h_, d_, et == 3);
  if (!rc && narrow) rc = ivfflat_rows(h_, 1);
  if (!rc && et == 4) {
    rc = ivfflat_sq8_rows(h_, 1);
    // brute_force_search on the trained model goes to the flat search over sq8 rows: its own switch, where the build has it
    const HIPFlatSq8RowsFn flat_sq8_rows = FindHIPFlatSq8Rows();
    narrow_brute_ = flat_sq8_rows != nullptr;
    if (!rc && flat_sq8_rows) rc = flat_sq8_rows(h_, 1);
  }
  if (!rc && narrow) {
    // brute_force_search and the search of an untrained model go to the flat search: its own switch, where the build has it
    const HIPFlatRowsFn flat_rows = FindHIPFlatRows();
    narrow_brute_ = flat_rows != nullptr;
    if (flat_rows) rc = flat_rows(h_, 1);
  }
  if (!rc) rc = gamma_hip_set_exact_ties(h_, pa.exact_ties ? 1 : 0);
  if (rc) {
    HLOG("device init failed: %s (%s)", gamma_hip_strerror(rc), gamma_hip_last_error(h_));
    return -1;
  }
  return 0;
}

RetrievalParameters *GammaIVFFlatHIPIndex::Parse(const std::string &parameters) {   // gamma_index_ivfflat.cc:188-242
  if (parameters == "") return new HIPIVFFlatRetrievalParameters(metric_type_);
  utils::JsonParser jp;
  if (jp.Parse(parameters.c_str())) {
    HLOG("parse retrieval parameters error: %s", parameters.c_str());
    return nullptr;
  }
  HIPIVFFlatRetrievalParameters *rp = new HIPIVFFlatRetrievalParameters();
  std::string mt;
  if (!jp.GetString("metric_type", mt)) {
    if (!strcasecmp("L2", mt.c_str())) rp->SetDistanceComputeType(DistanceComputeType::L2);
    else if (!strcasecmp("InnerProduct", mt.c_str())) rp->SetDistanceComputeType(DistanceComputeType::INNER_PRODUCT);
    else rp->SetDistanceComputeType(metric_type_);
  } else {
    rp->SetDistanceComputeType(metric_type_);
  }
  int v;
  if (!jp.GetInt("nprobe", v) && v > 0) rp->SetNprobe(v);
  if (!jp.GetInt("parallel_on_queries", v)) rp->SetParallelOnQueries(v != 0);
  if (!jp.GetInt("exact_ties", v)) rp->SetExactTies(v != 0 ? 1 : -1);
  return rp;
}

int GammaIVFFlatHIPIndex::SetTrainedCoarse(const float *coarse) {
  coarse_centroids_.assign(coarse, coarse + (size_t)nlist_ * d_);
  if (ForAll([&](gamma_hip_index *m) { return gamma_hip_ivfflat_set_trained(m, coarse_centroids_.data()); })) return -1;
  // several GPUs: no list sizes to balance yet -- lists are dealt round robin (Indexing balances by the training set's
  // assignment, Load by the dumped sizes)
  if (grp_ && gamma_hip_group_owner(grp_, 0) < 0 && gamma_hip_group_set_owners(grp_, nullptr)) return -1;
  is_trained_ = true;
  return 0;
}

int GammaIVFFlatHIPIndex::Indexing() {   // IndexIVFFlat::train == the coarse k-means (gamma_index_ivfflat.cc:244-303)
  if (is_trained_) return 0;
  std::vector<float> xt;
  size_t num = 0;
  if (TrainingSet(xt, num)) return -1;
  if (raw_sq8_ops_) {
    // "raw_dtype": "sq8": the store's per-dimension ranges from the training rows, before the coarse k-means and before any
    // row is mirrored (a narrow store's mirror is written from Add on)
    const int rc = raw_sq8_ops_->train(h_, (int64_t)num, xt.data());
    if (rc) {
      HLOG("sq8 range training failed: %s (%s)", gamma_hip_strerror(rc), gamma_hip_last_error(h_));
      return -1;
    }
  }
  if (TrainCoarse(num, xt.data())) return -1;   // once, on member 0; the centroids go to every member
  if (ForAll([&](gamma_hip_index *m) { return gamma_hip_ivfflat_set_trained(m, coarse_centroids_.data()); })) return -1;
  if (grp_) {
    // list -> GPU by the training set's list sizes, balanced greedily: the lists never move afterwards
    std::vector<int32_t> assign(num);
    int rc = gamma_hip_assign(h_, d_, (int64_t)num, xt.data(), nlist_, coarse_centroids_.data(), assign.data(), nullptr);
    std::vector<int64_t> weight(nlist_, 0);
    for (size_t i = 0; i < num && !rc; i++)
      if (assign[i] >= 0 && assign[i] < nlist_) weight[assign[i]]++;
    if (!rc) rc = gamma_hip_group_set_owners(grp_, weight.data());
    if (rc) {
      HLOG("training failed: %s (%s)", gamma_hip_strerror(rc), gamma_hip_group_last_error(grp_));
      return -1;
    }
  }
  is_trained_ = true;
  return 0;
}

int GammaIVFFlatHIPIndex::Search(RetrievalContext *retrieval_context, int n, const uint8_t *x, int k, float *distances,
                                 int64_t *ids) {
  HIPIVFFlatRetrievalParameters *rp = dynamic_cast<HIPIVFFlatRetrievalParameters *>(retrieval_context->RetrievalParams());
  HIPIVFFlatRetrievalParameters defaults(metric_type_);
  if (rp == nullptr) rp = &defaults;
  GammaSearchCondition *cond = dynamic_cast<GammaSearchCondition *>(retrieval_context);
  gamma_hip_search_params p;
  memset(&p, 0, sizeof(p));
  p.metric = rp->GetDistanceComputeType() == DistanceComputeType::INNER_PRODUCT ? GAMMA_HIP_METRIC_IP : GAMMA_HIP_METRIC_L2;
  p.min_score = cond ? cond->min_score : std::numeric_limits<float>::min();
  p.max_score = cond ? cond->max_score : std::numeric_limits<float>::max();
  p.coarse_mode = -1;
  p.exact_ties = rp->ExactTies();
  std::vector<gamma_hip_range_filter> rf;
  std::vector<gamma_hip_field_filter> ff;
  std::vector<gamma_hip_term_filter> tf;
  if (!(model_param_ && model_param_->device_filters &&
        columns_.Prepare(h_, cond, DocCountOf(this, (int64_t)vector_->MetaInfo()->Size()), p, ff, tf)))
    FillRangeFilters(cond, p, rf);
  const float *xq = reinterpret_cast<const float *>(x);
  int rc;
  if ((cond && cond->brute_force_search) || !is_trained_) {
    // (the reference's IVFFLAT has no brute-force branch; an untrained model would crash there.  Same service as HIPIVFPQ.)
    if (raw_sq8_ops_ && !is_trained_) {
      HLOG("HIPIVFFLAT: the search of an untrained model is not available with raw_dtype = sq8 (it has no ranges and holds no row)");
      return -1;
    }
    if (!narrow_brute_) {
      HLOG("HIPIVFFLAT: brute_force_search (and the search of an untrained model) over raw_dtype = %s needs flat search over narrow "
           "rows, which this build of the plugin does not have",
           raw_sq8_ops_ ? "sq8" : raw_f16_ ? "float16" : raw_i8_ == 2 ? "int8" : "uint8");
      return -1;
    }
    if (rawshard_) {
      // sharded rows (HIPIVFPQ's rule): member 0 mirrors the store until the first Add after training and serves the flat search
      // from it (raw_mu_ through the call); afterwards no device holds every row: refused, never a wrong answer
      std::lock_guard<std::mutex> g(raw_mu_);
      if (rows_sharded_) {
        HLOG("HIPIVFFLAT: brute_force_search is not available once the raw vectors are sharded (raw_placement = sharded)");
        return -3;
      }
      if (EnsureRawLocked((int64_t)vector_->MetaInfo()->Size())) return -1;
      rc = gamma_hip_flat_search(h_, &p, n, xq, k, distances, ids);
    } else {
      if (EnsureRaw((int64_t)vector_->MetaInfo()->Size())) return -1;
      rc = gamma_hip_flat_search(h_, &p, n, xq, k, distances, ids);   // (several devices, rows replicated: member 0 answers)
    }
  } else {
    // the reference takes retrieval_params->Nprobe() as it is (-1 when the request did not set it: a negative
    // allocation there, gamma_index_ivfflat.cc:405-410); the model's nprobe is the sane reading
    p.nprobe = (rp->Nprobe() > 0 && rp->Nprobe() <= nlist_) ? rp->Nprobe() : nprobe_;
    rc = grp_ ? group_search_(grp_, &p, n, xq, k, distances, ids) : gamma_hip_ivfflat_search(h_, &p, n, xq, k, distances, ids);
  }
  if (rc) {
    HLOG("search failed: %s (%s)", gamma_hip_strerror(rc), grp_ ? gamma_hip_group_last_error(grp_) : gamma_hip_last_error(h_));
    return rc;
  }
  WarnTiesNotHonoured(h_, grp_, &ties_said_);
  WarnBlasCorners(h_, grp_, &blas_said_);
  return 0;
}

// "ivfflat.index" in the reference's layout (gamma_index_ivfflat.cc:620-690; iwpq_io.h): a list's codes are its vectors
int GammaIVFFlatHIPIndex::Dump(const std::string &dir) {
  if (!is_trained_) return 0;
  const std::string index_dir = dir + "/" + vector_->MetaInfo()->AbsoluteName();
  if (mkdir(index_dir.c_str(), 0755) && errno != EEXIST) return -1;
  IwPQFile f;
  f.d = d_;
  f.ntotal = 0;
  f.metric = metric_type_ == DistanceComputeType::INNER_PRODUCT ? 0 : 1;
  f.nlist = (size_t)nlist_;
  f.nprobe = (size_t)nprobe_;
  f.coarse = coarse_centroids_;
  f.code_size = sizeof(float) * (size_t)d_;
  f.sizes.resize(nlist_);
  f.codes.resize(nlist_);
  f.ids.resize(nlist_);
  std::vector<uint8_t> dummy;
  for (int l = 0; l < nlist_; l++) {
    const int64_t len = grp_ ? gamma_hip_group_ivfpq_list_size(grp_, l) : gamma_hip_ivfpq_list_size(h_, l);
    if (len < 0) return -1;
    f.sizes[l] = (size_t)len;
    if (len == 0) continue;
    f.ids[l].resize(len);
    dummy.resize(len);
    if (grp_ ? gamma_hip_group_ivfpq_get_list(grp_, l, f.ids[l].data(), dummy.data())
             : gamma_hip_ivfpq_get_list(h_, l, f.ids[l].data(), dummy.data()))
      return -1;
    // the vectors of the list, from the engine's store (what the reference's lists hold)
    std::vector<int64_t> vids(len);
    for (int64_t i = 0; i < len; i++) vids[i] = f.ids[l][i] & 0x7fffffffffffffffLL;
    ScopeVectors sv;
    if (vector_->Gets(vids, sv)) return -1;
    f.codes[l].resize((size_t)len * f.code_size);
    for (int64_t i = 0; i < len; i++) memcpy(&f.codes[l][(size_t)i * f.code_size], sv.Get((int)i), f.code_size);
  }
  if (WriteIvFl(index_dir + "/ivfflat.index", f, indexed_vec_count_)) return -1;
  if (raw_sq8_ops_ && DumpSq8Ranges(index_dir)) return -1;   // a side file: ivfflat.index stays what the fp32 model writes
  return 0;
}

int GammaIVFFlatHIPIndex::Load(const std::string &dir) {
  const std::string path = dir + "/" + vector_->MetaInfo()->AbsoluteName() + "/ivfflat.index";
  FILE *probe = fopen(path.c_str(), "rb");
  if (!probe) return 0;   // it should train again after load
  fclose(probe);
  IwPQFile f;
  int indexed = 0;
  if (ReadIvFl(path, &f, &indexed)) return -1;
  if (f.d != d_ || (int)f.nlist != nlist_ || indexed < 0 || indexed > (int)vector_->MetaInfo()->Size()) return -1;
  // "raw_dtype": "sq8": the ranges come back before anything of the model changes and before the mirror is re-encoded below
  if (raw_sq8_ops_ && LoadSq8Ranges(dir + "/" + vector_->MetaInfo()->AbsoluteName())) return -1;
  if (raw_i8_ || raw_sq8_ops_) {
    // a byte or sq8 model: a pass over the rows it is about to mirror with the acceptance predicate first, so that a refused
    // row leaves the model as it was (untrained, no lists)
    std::lock_guard<std::mutex> g(raw_mu_);
    for (int64_t i0 = raw_uploaded_; i0 < indexed; i0 += 65536) {
      const int64_t nb = std::min<int64_t>(65536, indexed - i0);
      std::vector<int64_t> vids(nb);
      for (int64_t i = 0; i < nb; i++) vids[i] = i0 + i;
      ScopeVectors sv;
      if (vector_->Gets(vids, sv)) return -1;
      std::vector<float> buf((size_t)nb * d_);
      for (int64_t i = 0; i < nb; i++) memcpy(&buf[(size_t)i * d_], sv.Get((int)i), sizeof(float) * d_);
      if (!RowsStorable("load", buf.data(), nb)) return -1;
    }
  }
  if (grp_) {   // several GPUs: list -> GPU balanced by the dumped list sizes, before the lists come back
    std::vector<int64_t> weight(nlist_);
    for (int l = 0; l < nlist_; l++) weight[l] = (int64_t)f.sizes[l];
    if (gamma_hip_group_set_owners(grp_, weight.data())) return -1;
  }
  if (SetTrainedCoarse(f.coarse.data())) return -1;
  if (UploadEngineBitmap()) return -1;
  if (SyncVid2DocID((int64_t)vector_->MetaInfo()->Size())) return -1;
  metric_type_ = f.metric == 0 ? DistanceComputeType::INNER_PRODUCT : DistanceComputeType::L2;
  std::vector<uint8_t> dummy;
  for (int l = 0; l < nlist_; l++) {
    const size_t n = f.sizes[l];
    if (n == 0) continue;
    dummy.assign(n, 0);
    if (grp_ ? gamma_hip_group_ivfpq_add_keys(grp_, l, (int)n, f.ids[l].data(), dummy.data())
             : gamma_hip_ivfpq_add_keys(h_, l, (int)n, f.ids[l].data(), dummy.data()))
      return -1;
  }
  indexed_vec_count_ = indexed;
  const int64_t rows = std::min<int64_t>(indexed_vec_count_, (int64_t)vector_->MetaInfo()->Size());
  if (rawshard_) {   // sharded rows: every owner gets the rows of its lists back from the engine's store
    if (ShardRows() || PutRowsFromStore(rows)) return -1;
  } else if (EnsureRaw(rows)) {
    return -1;
  }
  return indexed_vec_count_;
}

}  // namespace tig_gamma
