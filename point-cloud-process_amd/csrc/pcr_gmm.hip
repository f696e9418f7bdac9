// Gaussian-mixture clustering: class GMM of Cluster_KMeans_GMM/GMM.py:13-71 (fit = EM with full covariances, predict = argmax of the
// weighted densities) on a device-resident cloud, in the log domain (semantics and the two deviations: include/pcr.h).
//
// Two streaming passes per EM iteration; each reads the 32-byte records once and never stores the responsibilities gamma:
//   gmm_estep_kernel   gamma under the CURRENT parameters; per component N_k = sum gamma and sum gamma x, and the log-likelihood of the
//                      current parameters.  The block that takes the last ticket applies the stop rule of GMM.py:61-63 to that
//                      log-likelihood (it is the previous iteration's nll) and writes the new means and weights;
//   gmm_cov_kernel     gamma AGAIN, by the same device function from the same parameters (bit-identical to the first pass), and the
//                      second moments about the new means.  Its last block divides, factors the covariances (Cholesky), builds the
//                      next iteration's constants and detects PCR_E_SINGULAR.
//   gmm_predict_kernel label (and responsibilities) by caller row, log-likelihood.
// A component's constants are 10 doubles (mean, the inverse of its Cholesky factor, log w - dim/2 log 2pi - sum log L_ii), broadcast
// from LDS.  A lane keeps GM_PTS points and, per point, the maximum m of the a_k and s = sum exp(a_k - m) in registers; components go
// by in chunks whose accumulators stay in registers, gamma_k = exp(a_k - m) / s evaluated per chunk.
// Sums: per lane over its points in order, wave totals on the DPP network (wave_total_f64), a fixed tree over the block's four waves,
// one slab per block in ctx->d_partials, and the last block adds the slabs in a fixed order.  No floating-point atomics, the block
// count depends on n alone: two runs give the same bits.  Loop state lives on the device; passes enqueued behind a stop are no-ops,
// and the host reads a 48-byte head once per chunk of GM_ITERS_PER_SYNC iterations.
#include <cmath>
#include <cstring>
#include <vector>
#include "pcr_internal.h"
#include "pcr_stream_fit.h"
#include "pcr_wave.h"

namespace {

constexpr int GM_MAX_K = PCR_GMM_MAX_K;
constexpr int GM_BLOCK = PCR_STREAM_BLOCK;
constexpr int GM_PTS = 4;                        // points per lane, in registers while the components go by
constexpr int GM_TILE = GM_PTS * GM_BLOCK;       // points per block: the block count is ceil(n / GM_TILE)
constexpr int GM_CHUNK = 8;                      // components per chunk of the E pass: 8 x (1 + dim) accumulators per lane
constexpr int GM_CHUNK_COV = 4;                  // of the covariance pass: 4 x 6
constexpr int GM_NC = 10;                        // doubles per component's constants
constexpr int GM_NSUM_MAX = GM_MAX_K * 6;        // sums per block slab: cov pass K * 6 (dim 3); E pass K * (1 + dim) + 1 <= 129
constexpr int GM_ITERS_PER_SYNC = 8;             // EM iterations enqueued per read-back of the loop state's head
constexpr double GM_LOG_2PI = 1.8378770664093454835606594728112;

// constants of a component: c[0..2] mean, c[3..8] rows of L^-1 (00, 10, 11, 20, 21, 22), c[9] = log w - dim/2 log 2pi - sum log L_ii.
// cov: xx, xy, xz, yy, yz, zz (dim 2: xx, xy, yy in slots 0, 1, 3).  false: a Cholesky pivot is not positive or not finite.
__host__ __device__ inline bool gmm_make_comp(int dim, const double* mu, const double* cov, double w, double* c) {
    const double d0 = cov[0];
    bool ok = d0 > 0.0 && d0 < INFINITY;
    const double l00 = sqrt(d0);
    const double l10 = cov[1] / l00;
    const double d1 = cov[3] - l10 * l10;
    ok = ok && d1 > 0.0 && d1 < INFINITY;
    const double l11 = sqrt(d1);
    const double i00 = 1.0 / l00, i11 = 1.0 / l11;
    const double i10 = -(l10 * i00) * i11;
    double i20 = 0.0, i21 = 0.0, i22 = 0.0, logdet = log(l00) + log(l11);
    if (dim == 3) {
        const double l20 = cov[2] / l00;
        const double l21 = (cov[4] - l20 * l10) / l11;
        const double d2 = cov[5] - (l20 * l20 + l21 * l21);
        ok = ok && d2 > 0.0 && d2 < INFINITY;
        const double l22 = sqrt(d2);
        i22 = 1.0 / l22;
        i21 = -(l21 * i11) * i22;
        i20 = -(l20 * i00 + l21 * i10) * i22;
        logdet = logdet + log(l22);
    }
    c[0] = mu[0]; c[1] = mu[1]; c[2] = dim == 3 ? mu[2] : 0.0;
    c[3] = i00; c[4] = i10; c[5] = i11; c[6] = i20; c[7] = i21; c[8] = i22;
    c[9] = (log(w) - 0.5 * (double)dim * GM_LOG_2PI) - logdet;
    return ok;
}

// a_k(x) = log w_k + log N(x; mu_k, Sigma_k).  THE density of this file: both passes, predict and pcr_gmm_log_density call it.
template <int DIM>
__host__ __device__ inline double gmm_log_density(const double* c, double x, double y, double z) {
    const double d0 = x - c[0], d1 = y - c[1];
    const double y0 = c[3] * d0, y1 = c[4] * d0 + c[5] * d1;
    double q = y0 * y0 + y1 * y1;
    if (DIM == 3) {
        const double d2 = z - c[2];
        const double y2 = (c[6] * d0 + c[7] * d1) + c[8] * d2;
        q = q + y2 * y2;
    }
    return c[9] - 0.5 * q;
}

// m = max_k a_k (lowest k on ties), s = sum_k exp(a_k - m): the point's log-likelihood is m + log s
template <int DIM>
__device__ inline void gmm_point_norm(const double* comp, int K, double x, double y, double z, double* m_out, double* s_out, int* arg_out) {
    double m = gmm_log_density<DIM>(comp, x, y, z);
    int arg = 0;
    for (int k = 1; k < K; ++k) {
        const double a = gmm_log_density<DIM>(comp + GM_NC * k, x, y, z);
        if (a > m) { m = a; arg = k; }
    }
    double s = 0.0;
    for (int k = 0; k < K; ++k) s += exp(gmm_log_density<DIM>(comp + GM_NC * k, x, y, z) - m);
    *m_out = m; *s_out = s; *arg_out = arg;
}
// gamma_k of a point whose normalisers are (m, s)
template <int DIM>
__device__ inline double gmm_resp(const double* c, double x, double y, double z, double m, double s) {
    return exp(gmm_log_density<DIM>(c, x, y, z) - m) / s;
}

// Loop state on the device.  The head (the first 48 bytes) is what the host reads per chunk of iterations.
struct __attribute__((aligned(16))) gmm_state {
    int it;              // completed EM iterations (M-steps)
    int stop;            // no further pass may run
    int status;          // PCR_OK or PCR_E_SINGULAR
    int converged;       // stopped by the rule of GMM.py:61
    int bad_component, bad_iter;   // PCR_E_SINGULAR: which component, in which iteration (1-based)
    int loop, max_iter;  // loop != 0: pcr_gmm_fit (stop rule, failure detection); 0: one step, whatever comes out
    double last_nll, loglik;       // GMM.py:27,63; log-likelihood of the current parameters as of the last E pass
    double tol, n_points;
    double mean[GM_MAX_K * 3], cov[GM_MAX_K * 6], weight[GM_MAX_K];   // current parameters
    double comp[GM_MAX_K * GM_NC];                                    // their constants
    double new_mean[GM_MAX_K * 3], new_weight[GM_MAX_K], nk[GM_MAX_K];   // E pass -> covariance pass
};
constexpr size_t GM_HEAD_BYTES = offsetof(gmm_state, tol);
static_assert(GM_HEAD_BYTES == 48, "head of the loop state");
static_assert(sizeof(gmm_state) <= PCR_SMALL_D2H_BYTES && sizeof(gmm_state) % 8 == 0, "state read back through pcr_d2h_small");

// host parameters -> state (one block): constants of every component, PCR_E_SINGULAR for the lowest component that has none
__global__ void __launch_bounds__(64) gmm_init_kernel(gmm_state* __restrict__ st, int K, int dim) {
    __shared__ int s_bad[GM_MAX_K];
    const int k = threadIdx.x;
    if (k < K) s_bad[k] = gmm_make_comp(dim, st->mean + 3 * k, st->cov + 6 * k, st->weight[k], st->comp + GM_NC * k) ? 0 : 1;
    __syncthreads();
    if (k != 0) return;
    for (int j = 0; j < K; ++j)
        if (s_bad[j]) { st->status = PCR_E_SINGULAR; st->stop = 1; st->bad_component = j; st->bad_iter = 0; return; }
}

// block_slab_sums (pcr_wave.h) with plain binary64 adds: one slab per block, the last block's fixed-order total in s_tot
__device__ inline bool gmm_block_sums(const double (*s_part)[GM_NSUM_MAX], int nsum, double* __restrict__ partials, unsigned int* __restrict__ ticket,
                                      double (*s_red)[GM_NSUM_MAX], double* s_tot) {
    return block_slab_sums<GM_NSUM_MAX>(s_part, nsum, partials, ticket, s_red, s_tot, [](double x, double y, int) { return x + y; });
}

// the constants of `st` into LDS (every pass, ahead of its tile load and the barrier)
__device__ inline void gmm_stage_comp(const gmm_state* __restrict__ st, int K, double* s_comp) {
    for (int t = threadIdx.x; t < K * GM_NC; t += GM_BLOCK) s_comp[t] = st->comp[t];
}

// E pass.  Slab layout: component k at [k * (1 + DIM), ...) = N_k, sum gamma x (, y, z); the log-likelihood at K * (1 + DIM).
template <int DIM>
__global__ void __launch_bounds__(GM_BLOCK)
gmm_estep_kernel(const pcr_pt* __restrict__ pts, long long n, int K, gmm_state* __restrict__ st, double* __restrict__ partials, unsigned int* __restrict__ ticket,
                 double* __restrict__ nll_hist) {
    constexpr int NT = 1 + DIM;
    __shared__ double s_comp[GM_MAX_K * GM_NC];
    __shared__ double s_part[4][GM_NSUM_MAX], s_red[8][GM_NSUM_MAX], s_tot[GM_NSUM_MAX];
    if (st->stop) return;
    double x[GM_PTS], y[GM_PTS], z[GM_PTS], m[GM_PTS], s[GM_PTS];
    bool valid[GM_PTS];
    gmm_stage_comp(st, K, s_comp);
    block_tile_load<GM_PTS, false>(pts, n, x, y, z, valid, nullptr);
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double ll = 0.0;
#pragma unroll
    for (int p = 0; p < GM_PTS; ++p) {
        int arg;
        gmm_point_norm<DIM>(s_comp, K, x[p], y[p], z[p], &m[p], &s[p], &arg);
        ll += valid[p] ? m[p] + log(s[p]) : 0.0;
    }
    ll = wave_total_f64(ll);
    if (lane == 63) s_part[wave][K * NT] = ll;
    for (int k0 = 0; k0 < K; k0 += GM_CHUNK) {
        double acc[GM_CHUNK][NT];
#pragma unroll
        for (int j = 0; j < GM_CHUNK; ++j)
#pragma unroll
            for (int c = 0; c < NT; ++c) acc[j][c] = 0.0;
#pragma unroll
        for (int p = 0; p < GM_PTS; ++p) {
#pragma unroll
            for (int j = 0; j < GM_CHUNK; ++j) {
                if (k0 + j < K) {   // uniform
                    const double g0 = gmm_resp<DIM>(s_comp + GM_NC * (k0 + j), x[p], y[p], z[p], m[p], s[p]);
                    const double g = valid[p] ? g0 : 0.0;
                    acc[j][0] += g;
                    acc[j][1] += g * x[p];
                    acc[j][2] += g * y[p];
                    if (DIM == 3) acc[j][NT - 1] += g * z[p];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < GM_CHUNK; ++j) {
#pragma unroll
            for (int c = 0; c < NT; ++c) {
                const double v = wave_total_f64(acc[j][c]);   // total in lane 63; every lane takes part
                if (lane == 63 && k0 + j < K) s_part[wave][(k0 + j) * NT + c] = v;
            }
        }
    }
    const int nsum = K * NT + 1;
    if (!gmm_block_sums(s_part, nsum, partials, ticket, s_red, s_tot)) return;

    // ---- the last block: the stop rule on the log-likelihood of the current parameters, then the new means and weights
    __shared__ int s_bad[GM_MAX_K];
    const int k = threadIdx.x;
    if (k < K) {
        const double nk = s_tot[k * NT];
        s_bad[k] = (nk > 0.0 && nk < INFINITY) ? 0 : 1;
        st->nk[k] = nk;
        st->new_weight[k] = nk / st->n_points;
        st->new_mean[3 * k] = s_tot[k * NT + 1] / nk;
        st->new_mean[3 * k + 1] = s_tot[k * NT + 2] / nk;
        st->new_mean[3 * k + 2] = DIM == 3 ? s_tot[k * NT + NT - 1] / nk : 0.0;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double loglik = s_tot[K * NT];
    st->loglik = loglik;
    if (!st->loop) return;
    const int it = st->it;
    if (it > 0) {   // GMM.py:56-63 for iteration `it`, whose parameters these are
        const double nll = -loglik;
        if (nll_hist) nll_hist[it - 1] = nll;
        if (st->last_nll - nll < st->tol) { st->converged = 1; st->stop = 1; return; }
        st->last_nll = nll;
        if (it >= st->max_iter) { st->stop = 1; return; }
    }
    for (int j = 0; j < K; ++j)
        if (s_bad[j]) { st->status = PCR_E_SINGULAR; st->stop = 1; st->bad_component = j; st->bad_iter = it + 1; return; }
}

// Covariance pass.  Slab layout: component k at [k * NT, ...) = sum gamma d_i d_j, (i, j) = xx, xy, (xz,) yy (, yz, zz), d = x - new mean.
template <int DIM>
__global__ void __launch_bounds__(GM_BLOCK)
gmm_cov_kernel(const pcr_pt* __restrict__ pts, long long n, int K, gmm_state* __restrict__ st, double* __restrict__ partials, unsigned int* __restrict__ ticket) {
    constexpr int NT = DIM * (DIM + 1) / 2;
    __shared__ double s_comp[GM_MAX_K * GM_NC], s_mean[GM_MAX_K * 3];
    __shared__ double s_part[4][GM_NSUM_MAX], s_red[8][GM_NSUM_MAX], s_tot[GM_NSUM_MAX];
    if (st->stop) return;
    double x[GM_PTS], y[GM_PTS], z[GM_PTS], m[GM_PTS], s[GM_PTS];
    bool valid[GM_PTS];
    for (int t = threadIdx.x; t < K * 3; t += GM_BLOCK) s_mean[t] = st->new_mean[t];
    gmm_stage_comp(st, K, s_comp);
    block_tile_load<GM_PTS, false>(pts, n, x, y, z, valid, nullptr);
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int p = 0; p < GM_PTS; ++p) {
        int arg;
        gmm_point_norm<DIM>(s_comp, K, x[p], y[p], z[p], &m[p], &s[p], &arg);
    }
    for (int k0 = 0; k0 < K; k0 += GM_CHUNK_COV) {
        double acc[GM_CHUNK_COV][NT];
#pragma unroll
        for (int j = 0; j < GM_CHUNK_COV; ++j)
#pragma unroll
            for (int c = 0; c < NT; ++c) acc[j][c] = 0.0;
#pragma unroll
        for (int p = 0; p < GM_PTS; ++p) {
#pragma unroll
            for (int j = 0; j < GM_CHUNK_COV; ++j) {
                if (k0 + j < K) {   // uniform
                    const double g0 = gmm_resp<DIM>(s_comp + GM_NC * (k0 + j), x[p], y[p], z[p], m[p], s[p]);
                    const double g = valid[p] ? g0 : 0.0;
                    const double dx = x[p] - s_mean[3 * (k0 + j)], dy = y[p] - s_mean[3 * (k0 + j) + 1];
                    if (DIM == 3) {
                        const double dz = z[p] - s_mean[3 * (k0 + j) + 2];
                        acc[j][0] += g * (dx * dx); acc[j][1] += g * (dx * dy); acc[j][2] += g * (dx * dz);
                        acc[j][NT - 3] += g * (dy * dy); acc[j][NT - 2] += g * (dy * dz); acc[j][NT - 1] += g * (dz * dz);
                    } else {
                        acc[j][0] += g * (dx * dx); acc[j][1] += g * (dx * dy); acc[j][2] += g * (dy * dy);
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < GM_CHUNK_COV; ++j) {
#pragma unroll
            for (int c = 0; c < NT; ++c) {
                const double v = wave_total_f64(acc[j][c]);
                if (lane == 63 && k0 + j < K) s_part[wave][(k0 + j) * NT + c] = v;
            }
        }
    }
    if (!gmm_block_sums(s_part, K * NT, partials, ticket, s_red, s_tot)) return;

    // ---- the last block: covariances about the new means, their factors, the next iteration's constants
    __shared__ int s_bad[GM_MAX_K];
    __shared__ double s_new[GM_MAX_K * GM_NC];
    const int k = threadIdx.x;
    double cov[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (k < K) {
        const double nk = st->nk[k];
        if (DIM == 3) {
#pragma unroll
            for (int c = 0; c < 6; ++c) cov[c] = s_tot[k * NT + c] / nk;
        } else {
            cov[0] = s_tot[k * NT] / nk; cov[1] = s_tot[k * NT + 1] / nk; cov[3] = s_tot[k * NT + 2] / nk;
        }
        s_bad[k] = gmm_make_comp(DIM, s_mean + 3 * k, cov, st->new_weight[k], s_new + GM_NC * k) ? 0 : 1;
    }
    __syncthreads();
    __shared__ int s_fail;
    if (threadIdx.x == 0) {
        s_fail = 0;
        if (st->loop) {
            for (int j = 0; j < K; ++j)
                if (s_bad[j]) { st->status = PCR_E_SINGULAR; st->stop = 1; st->bad_component = j; st->bad_iter = st->it + 1; s_fail = 1; break; }
        }
        if (!s_fail) st->it = st->it + 1;
    }
    __syncthreads();
    if (s_fail || k >= K) return;   // a failed iteration leaves the parameters of the one before
#pragma unroll
    for (int c = 0; c < 6; ++c) st->cov[6 * k + c] = cov[c];
#pragma unroll
    for (int c = 0; c < 3; ++c) st->mean[3 * k + c] = s_mean[3 * k + c];
    st->weight[k] = st->new_weight[k];
#pragma unroll
    for (int c = 0; c < GM_NC; ++c) st->comp[GM_NC * k + c] = s_new[GM_NC * k + c];
}

// label (lowest k on ties) and, if asked for, the responsibilities, by CALLER row (the records may be Morton-reordered: id is the
// row); the log-likelihood through the slabs like the E pass (one sum)
template <int DIM>
__global__ void __launch_bounds__(GM_BLOCK)
gmm_predict_kernel(const pcr_pt* __restrict__ pts, long long n, int K, gmm_state* __restrict__ st, double* __restrict__ partials, unsigned int* __restrict__ ticket,
                   int* __restrict__ labels, double* __restrict__ resp) {
    __shared__ double s_comp[GM_MAX_K * GM_NC];
    __shared__ double s_part[4][GM_NSUM_MAX], s_red[8][GM_NSUM_MAX], s_tot[GM_NSUM_MAX];
    if (st->stop) return;
    double x[GM_PTS], y[GM_PTS], z[GM_PTS];
    long long id[GM_PTS];
    bool valid[GM_PTS];
    gmm_stage_comp(st, K, s_comp);
    block_tile_load<GM_PTS, true>(pts, n, x, y, z, valid, id);
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double ll = 0.0;
#pragma unroll
    for (int p = 0; p < GM_PTS; ++p) {
        double m, s;
        int arg;
        gmm_point_norm<DIM>(s_comp, K, x[p], y[p], z[p], &m, &s, &arg);
        ll += valid[p] ? m + log(s) : 0.0;
        if (!valid[p]) continue;
        labels[id[p]] = arg;
        if (resp)
            for (int k = 0; k < K; ++k) resp[id[p] * K + k] = gmm_resp<DIM>(s_comp + GM_NC * k, x[p], y[p], z[p], m, s);
    }
    ll = wave_total_f64(ll);
    if (lane == 63) s_part[wave][0] = ll;
    if (!gmm_block_sums(s_part, 1, partials, ticket, s_red, s_tot)) return;
    if (threadIdx.x == 0) st->loglik = s_tot[0];
}

// (k, dim, dim) row-major <-> the 6 stored entries; the lower triangle is read, like numpy.linalg.cholesky
void cov_pack(int dim, const double* full, double* c6) {
    for (int i = 0; i < 6; ++i) c6[i] = 0.0;
    c6[0] = full[0]; c6[1] = full[dim]; c6[3] = full[dim + 1];
    if (dim == 3) { c6[2] = full[6]; c6[4] = full[7]; c6[5] = full[8]; }
}
void cov_unpack(int dim, const double* c6, double* full) {
    full[0] = c6[0]; full[1] = full[dim] = c6[1]; full[dim + 1] = c6[3];
    if (dim == 3) { full[2] = full[6] = c6[2]; full[5] = full[7] = c6[4]; full[8] = c6[5]; }
}

bool shape_ok(int k, int dim) { return k >= 1 && k <= GM_MAX_K && (dim == 2 || dim == 3); }

void state_from_host(gmm_state* h, int k, int dim, const double* means, const double* covs, const double* weights, int64_t n) {
    memset(h, 0, sizeof(*h));
    h->bad_component = -1;
    h->last_nll = INFINITY;
    h->n_points = (double)n;
    for (int j = 0; j < k; ++j) {
        for (int c = 0; c < dim; ++c) h->mean[3 * j + c] = means[j * dim + c];
        cov_pack(dim, covs + (size_t)j * dim * dim, h->cov + 6 * j);
        h->weight[j] = weights[j];
    }
}
void state_to_host(const gmm_state* h, int k, int dim, double* means, double* covs, double* weights) {
    for (int j = 0; j < k; ++j) {
        if (means) for (int c = 0; c < dim; ++c) means[j * dim + c] = h->mean[3 * j + c];
        if (covs) cov_unpack(dim, h->cov + 6 * j, covs + (size_t)j * dim * dim);
        if (weights) weights[j] = h->weight[j];
    }
}

// state uploaded and the constants built; the slabs sized for the largest pass
int gmm_begin(pcr_stream_fit* r, const pcr_cloud* cloud, int k, int dim, const gmm_state* h) {
    pcr_ctx* ctx = r->ctx;
    int rc;
    if ((rc = pcr_stream_begin(r, cloud->d, cloud->n, k, dim, GM_TILE, PCR_CW_GMM_TICKET, h, sizeof(gmm_state), GM_NSUM_MAX))) return rc;
    hipLaunchKernelGGL(gmm_init_kernel, dim3(1), dim3(64), 0, ctx->stream, r->st.as<gmm_state>(), k, dim);
    PCR_HIP(ctx, hipGetLastError());
    return PCR_OK;
}
int gmm_estep(pcr_stream_fit* r, double* d_hist) { return pcr_stream_launch(r, gmm_estep_kernel<2>, gmm_estep_kernel<3>, d_hist); }
int gmm_cov(pcr_stream_fit* r) { return pcr_stream_launch(r, gmm_cov_kernel<2>, gmm_cov_kernel<3>); }

}  // namespace

extern "C" {

void pcr_gmm_default_params(pcr_gmm_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->n_clusters = 1;
    p->dim = 3;
    p->max_iter = 50;   // GMM.py:14
    p->tol = 0.001;
}

int pcr_gmm_log_density(int dim, const double* x, const double* mean, const double* cov, double weight, double* a_out) {
    if (!x || !mean || !cov || !a_out || (dim != 2 && dim != 3) || !(weight > 0.0) || !std::isfinite(weight)) return PCR_E_INVALID;
    double c6[6], c[GM_NC];
    cov_pack(dim, cov, c6);
    if (!gmm_make_comp(dim, mean, c6, weight, c)) return PCR_E_SINGULAR;
    *a_out = dim == 3 ? gmm_log_density<3>(c, x[0], x[1], x[2]) : gmm_log_density<2>(c, x[0], x[1], 0.0);
    return PCR_OK;
}

int pcr_gmm_step(pcr_ctx* ctx, const pcr_cloud* cloud, int k, int dim, const double* means, const double* covs, const double* weights, double* means_out,
                 double* covs_out, double* weights_out, double* nk_out, double* loglik_out) {
    if (!ctx || !cloud || !means || !covs || !weights || !shape_ok(k, dim)) return PCR_E_INVALID;
    if (cloud->n <= 0) return PCR_E_EMPTY;
    hipSetDevice(ctx->device);
    std::vector<gmm_state> h(1);
    state_from_host(&h[0], k, dim, means, covs, weights, cloud->n);
    pcr_stream_fit r(ctx);
    int rc;
    if ((rc = gmm_begin(&r, cloud, k, dim, &h[0])) || (rc = gmm_estep(&r, nullptr)) || (rc = gmm_cov(&r))) return rc;
    if ((rc = pcr_d2h_small(ctx, &h[0], r.st.p, sizeof(gmm_state)))) return rc;
    if (h[0].status != PCR_OK) return h[0].status;
    state_to_host(&h[0], k, dim, means_out, covs_out, weights_out);
    if (nk_out) for (int j = 0; j < k; ++j) nk_out[j] = h[0].nk[j];
    if (loglik_out) *loglik_out = h[0].loglik;
    return PCR_OK;
}

int pcr_gmm_fit(pcr_ctx* ctx, const pcr_cloud* cloud, const pcr_gmm_params* params, const double* means0, double* means_out, double* covs_out,
                double* weights_out, double* nll_hist_out, pcr_gmm_result* result) {
    if (!ctx || !cloud || !params || !means0 || !result) return PCR_E_INVALID;
    const int k = params->n_clusters, dim = params->dim, max_iter = params->max_iter;
    if (!shape_ok(k, dim) || max_iter < 1 || std::isnan(params->tol)) return PCR_E_INVALID;
    if (cloud->n <= 0) return PCR_E_EMPTY;
    hipSetDevice(ctx->device);
    memset(result, 0, sizeof(*result));
    result->bad_component = -1;
    // GMM.py:20,26: identity covariances, weights 1 / k
    std::vector<double> covs0((size_t)k * dim * dim, 0.0), w0(k, 1.0 / (double)k);
    for (int j = 0; j < k; ++j)
        for (int c = 0; c < dim; ++c) covs0[((size_t)j * dim + c) * dim + c] = 1.0;
    std::vector<gmm_state> h(1);
    state_from_host(&h[0], k, dim, means0, covs0.data(), w0.data(), cloud->n);
    h[0].loop = 1;
    h[0].max_iter = max_iter;
    h[0].tol = params->tol;
    pcr_stream_fit r(ctx);
    pcr_dev_block d_hist(ctx);
    int rc;
    if ((rc = d_hist.alloc(sizeof(double) * max_iter))) return rc;
    PCR_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    if ((rc = gmm_begin(&r, cloud, k, dim, &h[0]))) return rc;
    // iteration i = E pass + covariance pass; the stop after iteration i is decided in the E pass of iteration i + 1, so a loop of
    // `iters` iterations costs 2 iters + 1 passes.  Passes behind a stop return at once.
    if ((rc = pcr_stream_loop(&r, max_iter + 1, GM_ITERS_PER_SYNC, GM_HEAD_BYTES, [&](int i) {
            const int e = gmm_estep(&r, d_hist.as<double>());
            return (e || i == max_iter) ? e : gmm_cov(&r);
        })))
        return rc;
    PCR_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    if ((rc = pcr_d2h_small(ctx, &h[0], r.st.p, sizeof(gmm_state)))) return rc;
    result->iters = h[0].it;
    result->converged = h[0].converged;
    result->bad_component = h[0].bad_component;
    result->bad_iter = h[0].bad_iter;
    result->passes = 2 * h[0].it + 1;
    if (h[0].status == PCR_OK) {
        result->nll = -h[0].loglik;
        state_to_host(&h[0], k, dim, means_out, covs_out, weights_out);
        if (nll_hist_out && h[0].it > 0) {
            PCR_HIP(ctx, hipMemcpyAsync(nll_hist_out, d_hist.p, sizeof(double) * h[0].it, hipMemcpyDeviceToHost, ctx->stream));
            PCR_HIP(ctx, pcr_sync(ctx->stream));
        }
    }
    if ((rc = pcr_events_ms(ctx, &result->device_ms))) return rc;
    return h[0].status;
}

int pcr_gmm_predict(pcr_ctx* ctx, const pcr_cloud* cloud, int k, int dim, const double* means, const double* covs, const double* weights, int32_t* labels_out,
                    double* resp_out, double* loglik_out) {
    if (!ctx || !cloud || !means || !covs || !weights || !labels_out || !shape_ok(k, dim)) return PCR_E_INVALID;
    const int64_t n = cloud->n;
    if (n <= 0) return PCR_E_EMPTY;
    hipSetDevice(ctx->device);
    std::vector<gmm_state> h(1);
    state_from_host(&h[0], k, dim, means, covs, weights, n);
    pcr_stream_fit r(ctx);
    pcr_dev_block d_labels(ctx), d_resp(ctx);
    int rc;
    if ((rc = d_labels.alloc(sizeof(int32_t) * n)) || (resp_out && (rc = d_resp.alloc(sizeof(double) * n * k)))) return rc;
    if ((rc = gmm_begin(&r, cloud, k, dim, &h[0]))) return rc;
    if ((rc = pcr_stream_launch(&r, gmm_predict_kernel<2>, gmm_predict_kernel<3>, d_labels.as<int>(), d_resp.as<double>()))) return rc;
    if ((rc = pcr_d2h_small(ctx, &h[0], r.st.p, GM_HEAD_BYTES))) return rc;
    if (h[0].status != PCR_OK) return h[0].status;
    if (loglik_out) *loglik_out = h[0].loglik;
    if ((rc = pcr_d2h_staged(ctx, labels_out, d_labels.p, sizeof(int32_t) * n))) return rc;
    if (resp_out && (rc = pcr_d2h_staged(ctx, resp_out, d_resp.p, sizeof(double) * n * k))) return rc;
    return PCR_OK;
}

}  // extern "C"
