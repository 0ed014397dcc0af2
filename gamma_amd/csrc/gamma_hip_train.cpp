// gamma_hip_train.cpp -- training on the device: faiss::Clustering::train (faiss:Clustering.cpp:255-560) the way
// GammaIVFPQIndex::Indexing runs it (index/impl/gamma_index_ivfpq.cc:272-354 -> IndexIVFPQ::train).
// The training set stays in HBM; per iteration the device assigns every point to its nearest centroid (the coarse
// quantizer's kernels: GEMM form from 20 points on, as faiss's IndexFlatL2::search) and sums every cluster's points --
// in ascending point order, one float accumulator per (cluster, dimension), which is compute_centroids' arithmetic --
// and the host does what is sequential and tiny: the random permutations (std::mt19937, faiss:utils/random.cpp), the
// stable grouping of the points by cluster, and split_clusters for clusters left empty.  Same subsampling, same
// initialisation, same sums, same splits as the library: oracle/gamma_oracle.c go_kmeans is the CPU statement of
// exactly this function (bit-identical results, tests/test_gpu_training.py) and is itself pinned against the
// compiled faiss (tests/test_training_cpu.py).
#include <random>

#include "binivf.h"
#include "gamma_hip_internal.h"
#include "opq.h"

using namespace ghi;

namespace {

// rand_perm, faiss:utils/random.cpp:136-146
void rand_perm(std::vector<int>& perm, size_t n, int64_t seed) {
    perm.resize(n);
    for (size_t i = 0; i < n; i++) perm[i] = (int)i;
    std::mt19937 mt((unsigned int)seed);
    for (size_t i = 0; i + 1 < n; i++) {
        const int i2 = (int)(i + mt() % (unsigned long)(int)(n - i));
        std::swap(perm[i], perm[i2]);
    }
}

// split_clusters, faiss:Clustering.cpp:220-268
int split_clusters(int d, int k, int64_t n, float* hassign, float* centroids) {
    int nsplit = 0;
    std::mt19937 mt(1234u);
    for (int ci = 0; ci < k; ci++) {
        if (hassign[ci] != 0) continue;
        int cj;
        for (cj = 0; 1; cj = (cj + 1) % k) {
            const float p = (float)(((double)hassign[cj] - 1.0) / (double)(float)(n - k));
            const float r = mt() / float(mt.max());
            if (r < p) break;
        }
        memcpy(centroids + (size_t)ci * d, centroids + (size_t)cj * d, sizeof(float) * d);
        for (int j = 0; j < d; j++) {
            float& a = centroids[(size_t)ci * d + j];
            float& b = centroids[(size_t)cj * d + j];
            if (j % 2 == 0) {
                a = (float)((double)a * (1 + 1 / 1024.));
                b = (float)((double)b * (1 - 1 / 1024.));
            } else {
                a = (float)((double)a * (1 - 1 / 1024.));
                b = (float)((double)b * (1 + 1 / 1024.));
            }
        }
        hassign[ci] = hassign[cj] / 2;
        hassign[cj] -= hassign[ci];
        nsplit++;
    }
    return nsplit;
}


// binary_to_real (faiss:utils/utils.cpp:634-638) of one code of d bits
void bin_decode_row(const uint8_t* c, int d, float* out) {
    for (int i = 0; i < d; i++) out[i] = (float)(2 * ((c[i >> 3] >> (i & 7)) & 1) - 1);
}

}  // namespace

namespace ghi {

// Clustering::train (x_in: n x d floats) or Clustering::train_encoded through IndexBinaryIVF's IndexLSH codec (codes_in:
// n codes of d bits, decoded to +-1 -- on the device for the training set, on the host for the k initial rows; the
// assignment searches blocks of decode_block_size = 32768 points, faiss:Clustering.cpp:378-393, so the exact form is
// chosen per block)
// hot_start (ProductQuantizer::Train_hot_start, faiss:impl/ProductQuantizer.cpp:224-232): `centroids` holds the initial
// centroids on entry instead of k points of the second permutation.  dev_x: the training set is ALREADY on the handle's
// device (n x d, contiguous; the caller keeps n <= k * max_points_per_centroid: nothing is subsampled) and is not
// uploaded; without a hot start its k initial rows are gathered on the device.  Calls without either behave as before.
static int kmeans_run(gamma_hip_index* h, int d, int64_t n, const float* x_in, const uint8_t* codes_in, int k, int niter,
                      int64_t seed, int max_points_per_centroid, float* centroids, float* objective, bool hot_start = false,
                      const float* dev_x = nullptr) {
    if (!h || d <= 0 || k <= 0 || niter < 0 || max_points_per_centroid <= 0 || (!x_in && !codes_in && !dev_x) || !centroids)
        return GAMMA_HIP_EINVAL;
    if (dev_x && (n > (int64_t)k * max_points_per_centroid || n <= k)) return GAMMA_HIP_EINVAL;
    if (codes_in && d % 8 != 0) return GAMMA_HIP_EINVAL;
    if (n < k) return fail(h, GAMMA_HIP_EINVAL, "k-means: fewer training points than clusters");
    SearchLock lk(h);
    GH_CHECK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    if (objective) *objective = 0.f;
    const size_t cs = (size_t)d / 8;
    // subsample_training_set (:92-120): the first k * max_points of a permutation
    std::vector<float> xsub;
    std::vector<uint8_t> csub;
    const float* x = x_in;
    const uint8_t* codes = codes_in;
    if (n > (int64_t)k * max_points_per_centroid) {
        std::vector<int> perm;
        rand_perm(perm, (size_t)n, seed);
        const int64_t n2 = (int64_t)k * max_points_per_centroid;
        if (codes) {
            csub.resize((size_t)n2 * cs);
            for (int64_t i = 0; i < n2; i++) memcpy(&csub[(size_t)i * cs], codes_in + (size_t)perm[i] * cs, cs);
            codes = csub.data();
        } else {
            xsub.resize((size_t)n2 * d);
            for (int64_t i = 0; i < n2; i++) memcpy(&xsub[(size_t)i * d], x_in + (size_t)perm[i] * d, sizeof(float) * d);
            x = xsub.data();
        }
        n = n2;
    }
    auto row = [&](int64_t i, float* out) {
        if (codes) bin_decode_row(codes + (size_t)i * cs, d, out);
        else memcpy(out, x + (size_t)i * d, sizeof(float) * d);
    };
    if (n == k) {   // :334-355
        for (int i = 0; i < k; i++) row(i, centroids + (size_t)i * d);
        return GAMMA_HIP_OK;
    }
    std::vector<int> init_perm;   // initial centroids: k points of a second permutation (:412-420)
    if (!hot_start) {
        rand_perm(init_perm, (size_t)n, seed + 1);
        if (!dev_x)
            for (int i = 0; i < k; i++) row(init_perm[i], centroids + (size_t)i * d);
    }
    if (niter == 0) return GAMMA_HIP_OK;
    // device state: the training set (resident for the whole run), the centroids, their norms
    DevBuf d_x, d_cen, d_cn, d_assign, d_dis, d_order, d_seg, d_has;   // (freed on every way out)
    if (!dev_x) GH_CHECK(h, d_x.ensure((size_t)n * d * sizeof(float)));
    GH_CHECK(h, d_cen.ensure((size_t)k * d * sizeof(float)));
    GH_CHECK(h, d_cn.ensure((size_t)k * sizeof(float)));
    GH_CHECK(h, d_assign.ensure((size_t)n * sizeof(int)));
    GH_CHECK(h, d_dis.ensure((size_t)n * sizeof(float)));
    GH_CHECK(h, d_order.ensure((size_t)n * sizeof(int)));
    GH_CHECK(h, d_seg.ensure((size_t)(k + 1) * sizeof(int)));
    GH_CHECK(h, d_has.ensure((size_t)k * sizeof(float)));
    if (codes) {   // the codes go up, the +-1 floats are made on the device
        DevBuf d_codes;
        GH_CHECK(h, d_codes.ensure((size_t)n * cs));
        GH_CHECK(h, hipMemcpyAsync(d_codes.p, codes, (size_t)n * cs, hipMemcpyHostToDevice, s));
        gh::launch_bin_decode(s, d_codes.as<uint8_t>(), n, d, d_x.as<float>());
        GH_CHECK(h, hipGetLastError());
        GH_CHECK(h, hipStreamSynchronize(s));
        d_codes.release();
    } else if (!dev_x) {
        GH_CHECK(h, hipMemcpyAsync(d_x.p, x, (size_t)n * d * sizeof(float), hipMemcpyHostToDevice, s));
    }
    const float* xd = dev_x ? dev_x : d_x.as<float>();   // the resident training set
    if (dev_x && !hot_start) {   // the k initial rows, gathered where the set is
        for (int i = 0; i < k; i++)
            GH_CHECK(h, hipMemcpyAsync(d_cen.as<float>() + (size_t)i * d, dev_x + (size_t)init_perm[i] * d, (size_t)d * sizeof(float),
                                       hipMemcpyDeviceToDevice, s));
    } else {
        GH_CHECK(h, hipMemcpyAsync(d_cen.p, centroids, (size_t)k * d * sizeof(float), hipMemcpyHostToDevice, s));
    }
    int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(n, (int64_t)(h->dist_budget_bytes / ((size_t)k * sizeof(float)))));
    if (codes) chunk = std::min<int64_t>(chunk, 32768);   // decode_block_size: one index.search per block
    GH_CHECK(h, h->w_mat.ensure((size_t)chunk * k * sizeof(float)));
    std::vector<int> assign(n), order(n), seg(k + 1);
    std::vector<float> hassign(k), dis;
    // IndexFlatL2::search: the exact form below 20 queries (faiss:utils/distances.cpp:346) -- of the whole call, or of
    // each decode block
    const bool exact_all = n < 20;
    if (!exact_all && blas_form_not_restated(n, k, d)) h->blas_unrestated++;
    for (int it = 0; it < niter; it++) {
        // index.search(nx, x, 1, dis, assign)
        gh::launch_row_norms(s, d_cen.as<float>(), k, d, d_cn.as<float>());
        for (int64_t i0 = 0; i0 < n; i0 += chunk) {
            const int64_t nc = std::min(chunk, n - i0);
            const bool exact = codes ? nc < 20 : exact_all;
            if (exact) gh::launch_pairwise(s, true, xd + i0 * d, (int)nc, d, d_cen.as<float>(), k, h->w_mat.as<float>(), k);
            else gh::launch_l2_gemmform(s, xd + i0 * d, (int)nc, d, d_cen.as<float>(), k, nullptr, d_cn.as<float>(),
                                        h->w_mat.as<float>(), k, true);
            gh::launch_select_topk(s, true, h->w_mat.as<float>(), k, nullptr, k, k, (int)nc, 1, d_dis.as<float>() + i0,
                                   d_assign.as<int>() + i0);
        }
        GH_CHECK(h, hipGetLastError());
        GH_CHECK(h, hipMemcpyAsync(assign.data(), d_assign.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, s));
        if (it == niter - 1 && objective) {
            dis.resize(n);
            GH_CHECK(h, hipMemcpyAsync(dis.data(), d_dis.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, s));
        }
        GH_CHECK(h, hipStreamSynchronize(s));
        // the points of every cluster in ascending point order (a stable counting sort): compute_centroids adds them
        // to the cluster's accumulators in exactly that order (:160-189)
        std::fill(seg.begin(), seg.end(), 0);
        for (int64_t i = 0; i < n; i++) {
            if (assign[i] < 0 || assign[i] >= k) return fail(h, GAMMA_HIP_EDEVICE, "k-means: bad assignment");
            seg[assign[i] + 1]++;
        }
        for (int c = 0; c < k; c++) seg[c + 1] += seg[c];
        {
            std::vector<int> at(seg.begin(), seg.end() - 1);
            for (int64_t i = 0; i < n; i++) order[at[assign[i]]++] = (int)i;
        }
        GH_CHECK(h, hipMemcpyAsync(d_order.p, order.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
        GH_CHECK(h, hipMemcpyAsync(d_seg.p, seg.data(), (size_t)(k + 1) * sizeof(int), hipMemcpyHostToDevice, s));
        gh::launch_centroid_update(s, xd, d, d_order.as<int>(), d_seg.as<int>(), k, d_cen.as<float>(), d_has.as<float>());
        GH_CHECK(h, hipGetLastError());
        // clusters left empty are re-seeded from large ones on the host (rare: a download of the centroids only then)
        bool any_empty = false;
        for (int c = 0; c < k; c++) {
            hassign[c] = (float)(seg[c + 1] - seg[c]);
            any_empty |= seg[c + 1] == seg[c];
        }
        if (any_empty) {
            GH_CHECK(h, hipMemcpyAsync(centroids, d_cen.p, (size_t)k * d * sizeof(float), hipMemcpyDeviceToHost, s));
            GH_CHECK(h, hipStreamSynchronize(s));
            split_clusters(d, k, n, hassign.data(), centroids);
            GH_CHECK(h, hipMemcpyAsync(d_cen.p, centroids, (size_t)k * d * sizeof(float), hipMemcpyHostToDevice, s));
        }
    }
    GH_CHECK(h, hipMemcpyAsync(centroids, d_cen.p, (size_t)k * d * sizeof(float), hipMemcpyDeviceToHost, s));
    GH_CHECK(h, hipStreamSynchronize(s));
    if (objective && !dis.empty()) {
        float obj = 0;   // :478-481, float accumulation in point order
        for (int64_t j = 0; j < n; j++) obj += dis[j];
        *objective = obj;
    }
    return GAMMA_HIP_OK;
}

}  // namespace ghi


// ---- OPQ training (gamma_hip_opq_train) --------------------------------------------------------------------------------------
namespace {

// rows of a d x d matrix made orthonormal in double (modified Gram-Schmidt, every row projected twice); a row that
// vanishes against its predecessors is replaced by the unit vector that is least represented so far
void orthonormalise_rows(std::vector<double>& q, int d) {
    for (int i = 0; i < d; i++) {
        double* r = &q[(size_t)i * d];
        for (int attempt = 0; attempt < 2 + d; attempt++) {
            double n0 = 0;
            for (int t = 0; t < d; t++) n0 += r[t] * r[t];
            for (int pass = 0; pass < 2; pass++)
                for (int j = 0; j < i; j++) {
                    const double* p = &q[(size_t)j * d];
                    double dot = 0;
                    for (int t = 0; t < d; t++) dot += r[t] * p[t];
                    for (int t = 0; t < d; t++) r[t] -= dot * p[t];
                }
            double nn = 0;
            for (int t = 0; t < d; t++) nn += r[t] * r[t];
            if (nn > 1e-20 && nn > 1e-24 * n0) {
                const double inv = 1.0 / sqrt(nn);
                for (int t = 0; t < d; t++) r[t] *= inv;
                break;
            }
            for (int t = 0; t < d; t++) r[t] = 0;   // (rank-deficient input) try the unit vectors in turn
            r[(i + attempt) % d] = 1.0;
        }
    }
}

// the orthogonal polar factor U V^T of C = U S V^T (d x d, row-major, double): one-sided Jacobi (Hestenes) on the columns
// of G = C until they are mutually orthogonal, G = U S with V the accumulated rotations; columns of U that belong to a
// vanishing singular value (a rank-deficient cross-product) are completed by orthonormalise_rows afterwards.
// out: d x d, orthonormal in double.  false: the sweeps did not converge.
bool polar_factor(const std::vector<double>& C, int d, std::vector<double>& out) {
    // column-major copies: column j of G / V is contiguous
    std::vector<double> G((size_t)d * d), V((size_t)d * d, 0.0);
    for (int i = 0; i < d; i++)
        for (int j = 0; j < d; j++) G[(size_t)j * d + i] = C[(size_t)i * d + j];
    for (int j = 0; j < d; j++) V[(size_t)j * d + j] = 1.0;
    double frob = 0;
    for (double v : G) frob += v * v;
    const double tiny = 1e-28 * frob;   // columns of a vanishing singular value: left alone (completed below)
    bool converged = false;
    for (int sweep = 0; sweep < 60 && !converged; sweep++) {
        converged = true;
        for (int p = 0; p < d - 1; p++)
            for (int q = p + 1; q < d; q++) {
                double* gp = &G[(size_t)p * d];
                double* gq = &G[(size_t)q * d];
                double a = 0, b = 0, c = 0;
                for (int t = 0; t < d; t++) {
                    a += gp[t] * gp[t];
                    b += gq[t] * gq[t];
                    c += gp[t] * gq[t];
                }
                if (a <= tiny || b <= tiny || fabs(c) <= 1e-13 * sqrt(a * b)) continue;
                converged = false;
                const double zeta = (b - a) / (2.0 * c);
                const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
                double* vp = &V[(size_t)p * d];
                double* vq = &V[(size_t)q * d];
                for (int k = 0; k < d; k++) {
                    const double x0 = gp[k], y0 = gq[k];
                    gp[k] = cs * x0 - sn * y0;
                    gq[k] = sn * x0 + cs * y0;
                    const double x1 = vp[k], y1 = vq[k];
                    vp[k] = cs * x1 - sn * y1;
                    vq[k] = sn * x1 + cs * y1;
                }
            }
    }
    if (!converged) return false;
    // U: the normalised columns of G; a vanishing column stays zero and is completed below
    double smax = 0;
    std::vector<double> nrm(d);
    for (int j = 0; j < d; j++) {
        double a = 0;
        for (int t = 0; t < d; t++) a += G[(size_t)j * d + t] * G[(size_t)j * d + t];
        nrm[j] = sqrt(a);
        smax = std::max(smax, nrm[j]);
    }
    // complete U in the space of its columns: rows of `ut` = columns of U
    std::vector<double> ut((size_t)d * d, 0.0);
    std::vector<int> order;
    for (int j = 0; j < d; j++)
        if (nrm[j] > 1e-12 * smax && nrm[j] > 0) order.push_back(j);
    for (int j = 0; j < d; j++)
        if (!(nrm[j] > 1e-12 * smax && nrm[j] > 0)) order.push_back(j);
    std::vector<double> uo((size_t)d * d, 0.0);   // rows in `order`: the well-defined columns first
    for (int r = 0; r < d; r++) {
        const int j = order[r];
        if (nrm[j] > 1e-12 * smax && nrm[j] > 0)
            for (int t = 0; t < d; t++) uo[(size_t)r * d + t] = G[(size_t)j * d + t] / nrm[j];
    }
    orthonormalise_rows(uo, d);
    for (int r = 0; r < d; r++) memcpy(&ut[(size_t)order[r] * d], &uo[(size_t)r * d], sizeof(double) * d);
    // Q = U V^T: Q[i][j] = sum_k U[i][k] V[j][k] = sum_k ut[k][i] * V(col k)[j]
    out.assign((size_t)d * d, 0.0);
    for (int k = 0; k < d; k++) {
        const double* uk = &ut[(size_t)k * d];
        const double* vk = &V[(size_t)k * d];
        for (int i = 0; i < d; i++) {
            const double u = uk[i];
            double* o = &out[(size_t)i * d];
            for (int j = 0; j < d; j++) o[j] += u * vk[j];
        }
    }
    orthonormalise_rows(out, d);   // the finish: orthonormal in double, rounded once to fp32 by the caller
    return true;
}

}  // namespace

extern "C" void gamma_hip_rand_perm(int32_t* perm, int64_t n, int64_t seed) {
    std::vector<int> p;
    rand_perm(p, (size_t)std::max<int64_t>(n, 0), seed);
    for (int64_t i = 0; i < n; i++) perm[i] = p[i];
}

extern "C" {

int gamma_hip_kmeans(gamma_hip_index* h, int d, int64_t n, const float* x_in, int k, int niter, int64_t seed,
                     int max_points_per_centroid, float* centroids, float* objective) {
    if (!x_in) return GAMMA_HIP_EINVAL;
    return kmeans_run(h, d, n, x_in, nullptr, k, niter, seed, max_points_per_centroid, centroids, objective);
}

// IndexBinaryIVF::train as GammaIndexBinaryIVF configures it (gamma_index_binary_ivf.cc:90-124,208-266;
// faiss:IndexBinaryIVF.cpp:241-280): Clustering(nbits, nlist) with niter 10, seed 1234, 256 points per centroid, trained
// on the codes through the IndexLSH codec (+-1 floats), then real_to_binary (faiss:utils/utils.cpp:640-650: bit set only
// for a component > 0).  codes: n x nbits / 8 bytes; centroid_codes: nlist x nbits / 8 bytes out.
int gamma_hip_binivf_train(gamma_hip_index* h, int nbits, int64_t n, const uint8_t* codes, int nlist, uint8_t* centroid_codes) {
    if (!h || nbits <= 0 || nbits % 8 != 0 || nlist <= 0 || !codes || !centroid_codes) return GAMMA_HIP_EINVAL;
    std::vector<float> cen((size_t)nlist * nbits);
    GH_TRY(kmeans_run(h, nbits, n, nullptr, codes, nlist, 10, 1234, 256, cen.data(), nullptr));
    const int cs = nbits / 8;
    for (int64_t i = 0; i < (int64_t)nlist * cs; i++) {
        uint8_t b = 0;
        for (int j = 0; j < 8; j++)
            if (cen[(size_t)i * 8 + j] > 0) b |= (uint8_t)(1 << j);
        centroid_codes[i] = b;
    }
    return GAMMA_HIP_OK;
}

// IndexIVFPQ::train as GammaIVFPQIndex::Indexing configures it (index/impl/gamma_index_ivfpq.cc:172-185,272-354):
// train_q1 -- Clustering(d, nlist) with cp.niter = 10, seed 1234, max_points_per_centroid 256 -- then
// train_residual_o (faiss:IndexIVFPQ.cpp:67-106): at most 256 * 256 points (fvecs_maybe_subsample with pq.cp.seed =
// 1234), their residuals to the nearest coarse centroid (by_residual), and ProductQuantizer::train: one
// Clustering(dsub, 256, niter 25) per sub-quantizer.  coarse: nlist*d, pq: M*256*(d/M) fp32 host out.
// On a handle initialised as 4-bit (gamma_hip_ivfpq4_init) ksub is 16: at most 256 * 16 points
// (pq.cp.max_points_per_centroid * pq.ksub, faiss:IndexIVFPQ.cpp:67-131), Clustering(dsub, 16, niter 25), pq: M*16*(d/M).
int gamma_hip_ivfpq_train(gamma_hip_index* h, int d, int64_t n, const float* x, int nlist, int M, float* coarse, float* pq) {
    if (!h || d <= 0 || nlist <= 0 || M <= 0 || d % M != 0 || !x || !coarse || !pq) return GAMMA_HIP_EINVAL;
    int rc = gamma_hip_kmeans(h, d, n, x, nlist, 10, 1234, 256, coarse, nullptr);
    if (rc) return rc;
    int ksub = 256;
    {
        std::lock_guard<std::mutex> g(h->mu);
        if (h->ivf_init && !h->ivfflat) ksub = h->ksub;
    }
    const int64_t nmax = 256 * (int64_t)ksub;
    std::vector<float> subset;
    const float* xs = x;
    int64_t ns = n;
    if (n > nmax) {
        std::vector<int> perm;
        rand_perm(perm, (size_t)n, 1234);
        subset.resize((size_t)nmax * d);
        for (int64_t i = 0; i < nmax; i++) memcpy(&subset[(size_t)i * d], x + (size_t)perm[i] * d, sizeof(float) * d);
        xs = subset.data();
        ns = nmax;
    }
    std::vector<int32_t> assign((size_t)ns);
    rc = gamma_hip_assign(h, d, ns, xs, nlist, coarse, assign.data(), nullptr);
    if (rc) return rc;
    const int dsub = d / M;
    std::vector<float> slice((size_t)ns * dsub);
    for (int m = 0; m < M; m++) {
        for (int64_t i = 0; i < ns; i++) {
            if (assign[i] < 0 || assign[i] >= nlist) return fail(h, GAMMA_HIP_EDEVICE, "training: bad assignment");
            const float* xi = xs + (size_t)i * d + m * dsub;
            const float* c = coarse + (size_t)assign[i] * d + m * dsub;
            for (int t = 0; t < dsub; t++) slice[(size_t)i * dsub + t] = xi[t] - c[t];
        }
        rc = gamma_hip_kmeans(h, dsub, ns, slice.data(), ksub, 25, 1234, 256, pq + (size_t)m * ksub * dsub, nullptr);
        if (rc) return rc;
    }
    return GAMMA_HIP_OK;
}


// OPQMatrix::train (faiss:VectorTransform.cpp:986-1200) as GammaIVFPQIndex::Init configures it -- OPQMatrix(d, M_opq, d):
// niter 50, niter_pq 4, niter_pq_0 40, max_train_points 256 * 256 (VectorTransform.h:213-222) -- with the training set
// resident on the device.  Structure and constants are the library's; the bits are not (its sgeqrf / sgesvd are not
// reproducible across thread counts, :997-1012): the quality is what tests/test_gpu_opq_train.py holds against it.
//   set-up   fvecs_maybe_subsample to 65536 points (rand_perm, seed 1234), centred with float sums in point order, a
//            random orthonormal start (std::mt19937(1234), Box-Muller, Gram-Schmidt in double)
//   niter x  rotate (opq.hip, the apply kernel) | per sub-quantizer: its columns as a contiguous set, a 256-centroid
//            k-means (40 iterations in the first alternation from a fresh start, 4 afterwards from the previous centroids,
//            max_points_per_centroid 1000), the final assignment, the decode | the d x d cross-product reconstruction^T x
//            set in double | its orthogonal polar factor (one-sided Jacobi in double on the host) as the next rotation
// A_out: d x d row-major (xt = A x).  objective_out (may be NULL): the mean squared PQ error of the last alternation's
// encode, from the k-means' own assignment distances.
int gamma_hip_opq_train(gamma_hip_index* h, int d, int64_t n, const float* x, int M_opq, int niter, float* A_out,
                        float* objective_out) {
    if (!h || d <= 0 || M_opq <= 0 || !x || !A_out) return GAMMA_HIP_EINVAL;
    if (d % M_opq != 0) return fail(h, GAMMA_HIP_EINVAL, "opq_train: d is not a multiple of the number of sub-quantizers");
    const int ksub = 256, ds = d / M_opq;
    if (n < ksub) return fail(h, GAMMA_HIP_EINVAL, "opq_train: fewer than 256 training points (one per PQ centroid)");
    if (niter <= 0) niter = 50;
    // subsample (fvecs_maybe_subsample, faiss:utils/utils.cpp: rand_perm(n, seed 1234), the first max_train_points)
    const int64_t nmax = 65536;
    std::vector<float> xt;
    if (n > nmax) {
        std::vector<int> perm;
        rand_perm(perm, (size_t)n, 1234);
        xt.resize((size_t)nmax * d);
        for (int64_t i = 0; i < nmax; i++) memcpy(&xt[(size_t)i * d], x + (size_t)perm[i] * d, sizeof(float) * d);
        n = nmax;
    } else {
        xt.assign(x, x + (size_t)n * d);
    }
    {   // centre (:1023-1041)
        std::vector<float> sum(d, 0.f);
        for (int64_t i = 0; i < n; i++)
            for (int j = 0; j < d; j++) sum[j] += xt[(size_t)i * d + j];
        for (int j = 0; j < d; j++) sum[j] /= n;
        for (int64_t i = 0; i < n; i++)
            for (int j = 0; j < d; j++) xt[(size_t)i * d + j] -= sum[j];
    }
    std::vector<double> Q((size_t)d * d);
    {   // the start
        std::mt19937 mt(1234u);
        for (size_t i = 0; i < Q.size(); i += 2) {
            const double u1 = (mt() + 1.0) / 4294967297.0, u2 = mt() / 4294967296.0;
            const double r = sqrt(-2.0 * log(u1));
            Q[i] = r * cos(2.0 * 3.14159265358979323846 * u2);
            if (i + 1 < Q.size()) Q[i + 1] = r * sin(2.0 * 3.14159265358979323846 * u2);
        }
        orthonormalise_rows(Q, d);
    }
    std::vector<float> A((size_t)d * d);
    for (size_t i = 0; i < A.size(); i++) A[i] = (float)Q[i];

    DevBuf d_x, d_xp, d_rec, d_A, d_slice, d_cen, d_cn, d_assign, d_dis, d_P, d_C;   // (freed on every way out)
    hipStream_t s = h->stream;
    {
        SearchLock lk(h);
        GH_CHECK(h, hipSetDevice(h->device));
        GH_CHECK(h, d_x.ensure((size_t)n * d * sizeof(float)));
        GH_CHECK(h, d_xp.ensure((size_t)n * d * sizeof(float)));
        GH_CHECK(h, d_rec.ensure((size_t)n * d * sizeof(float)));
        GH_CHECK(h, d_A.ensure((size_t)d * d * sizeof(float)));
        GH_CHECK(h, d_slice.ensure((size_t)n * ds * sizeof(float)));
        GH_CHECK(h, d_cen.ensure((size_t)ksub * ds * sizeof(float)));
        GH_CHECK(h, d_cn.ensure((size_t)ksub * sizeof(float)));
        GH_CHECK(h, d_assign.ensure((size_t)n * sizeof(int)));
        GH_CHECK(h, d_dis.ensure((size_t)n * sizeof(float)));
        GH_CHECK(h, d_P.ensure((size_t)gh::opq_cross_blocks(n) * d * d * sizeof(double)));
        GH_CHECK(h, d_C.ensure((size_t)d * d * sizeof(double)));
        GH_CHECK(h, hipMemcpyAsync(d_x.p, xt.data(), (size_t)n * d * sizeof(float), hipMemcpyHostToDevice, s));
        GH_CHECK(h, hipStreamSynchronize(s));
    }
    std::vector<float> cen((size_t)M_opq * ksub * ds), dis((size_t)n);
    std::vector<double> C((size_t)d * d);
    double err = 0;
    for (int it = 0; it < niter; it++) {
        {
            SearchLock lk(h);
            GH_CHECK(h, hipSetDevice(h->device));
            GH_CHECK(h, hipMemcpyAsync(d_A.p, A.data(), (size_t)d * d * sizeof(float), hipMemcpyHostToDevice, s));
            gh::launch_opq_apply(s, d_A.as<float>(), d, d_x.as<float>(), n, d_xp.as<float>());
            GH_CHECK(h, hipGetLastError());
            GH_CHECK(h, hipStreamSynchronize(s));
        }
        err = 0;
        for (int m = 0; m < M_opq; m++) {
            float* cm = &cen[(size_t)m * ksub * ds];
            {
                SearchLock lk(h);
                GH_CHECK(h, hipSetDevice(h->device));
                gh::launch_opq_slice(s, d_xp.as<float>(), n, d, m * ds, ds, d_slice.as<float>());
                GH_CHECK(h, hipGetLastError());
                GH_CHECK(h, hipStreamSynchronize(s));
            }
            if (n == ksub) {   // Clustering::train copies the points when there is one per centroid
                SearchLock lk(h);
                GH_CHECK(h, hipSetDevice(h->device));
                GH_CHECK(h, hipMemcpyAsync(cm, d_slice.p, (size_t)ksub * ds * sizeof(float), hipMemcpyDeviceToHost, s));
                GH_CHECK(h, hipStreamSynchronize(s));
            } else if (it == 0) {
                // the first alternation: a fresh 40-iteration k-means (its initial rows are gathered on the device)
                GH_TRY(kmeans_run(h, ds, n, nullptr, nullptr, ksub, 40, 1234, 1000, cm, nullptr, false, d_slice.as<float>()));
            } else {
                GH_TRY(kmeans_run(h, ds, n, nullptr, nullptr, ksub, 4, 1234, 1000, cm, nullptr, true, d_slice.as<float>()));
            }
            // encode + decode: the nearest final centroid of every point (the coarse quantizer's kernels), its row back
            SearchLock lk(h);
            GH_CHECK(h, hipSetDevice(h->device));
            GH_CHECK(h, hipMemcpyAsync(d_cen.p, cm, (size_t)ksub * ds * sizeof(float), hipMemcpyHostToDevice, s));
            gh::launch_row_norms(s, d_cen.as<float>(), ksub, ds, d_cn.as<float>());
            const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(n, (int64_t)(h->dist_budget_bytes / ((size_t)ksub * sizeof(float)))));
            GH_CHECK(h, h->w_mat.ensure((size_t)chunk * ksub * sizeof(float)));
            for (int64_t i0 = 0; i0 < n; i0 += chunk) {
                const int64_t nc = std::min(chunk, n - i0);
                gh::launch_l2_gemmform(s, d_slice.as<float>() + i0 * ds, (int)nc, ds, d_cen.as<float>(), ksub, nullptr, d_cn.as<float>(),
                                       h->w_mat.as<float>(), ksub, true);
                gh::launch_select_topk(s, true, h->w_mat.as<float>(), ksub, nullptr, ksub, ksub, (int)nc, 1, d_dis.as<float>() + i0,
                                       d_assign.as<int>() + i0);
            }
            gh::launch_opq_recons(s, d_cen.as<float>(), d_assign.as<int>(), ksub, n, d, m * ds, ds, d_rec.as<float>());
            GH_CHECK(h, hipGetLastError());
            GH_CHECK(h, hipMemcpyAsync(dis.data(), d_dis.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, s));
            GH_CHECK(h, hipStreamSynchronize(s));
            for (int64_t i = 0; i < n; i++) err += dis[i];
        }
        {
            SearchLock lk(h);
            GH_CHECK(h, hipSetDevice(h->device));
            gh::launch_opq_cross(s, d_rec.as<float>(), d_x.as<float>(), n, d, d_P.as<double>(), d_C.as<double>());
            GH_CHECK(h, hipGetLastError());
            GH_CHECK(h, hipMemcpyAsync(C.data(), d_C.p, (size_t)d * d * sizeof(double), hipMemcpyDeviceToHost, s));
            GH_CHECK(h, hipStreamSynchronize(s));
        }
        if (!polar_factor(C, d, Q)) return fail(h, GAMMA_HIP_EDEVICE, "opq_train: the Jacobi sweeps of the polar factor did not converge");
        for (size_t i = 0; i < A.size(); i++) A[i] = (float)Q[i];
    }
    memcpy(A_out, A.data(), A.size() * sizeof(float));
    if (objective_out) *objective_out = (float)(err / (double)n);
    return GAMMA_HIP_OK;
}

}  // extern "C"
