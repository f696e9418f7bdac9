// K-Means clustering (Lloyd's iteration): class K_Means of Cluster_KMeans_GMM/compare_cluster.py:16,105,164-170 on a device-resident
// cloud.  The reference's KMeans.py is not in its tree; the semantics are the ones include/pcr.h states.
//
// One streaming pass over the 32-byte records per iteration:
//   kmeans_assign_kernel  label = argmin_k d2 under the CURRENT centres (direct form, lowest k on ties), per cluster the exact count
//                         N_k and S_k = sum x, and the inertia of the current centres.  The block that takes the last ticket divides,
//                         keeps the centre of an empty cluster, applies the stop rule, writes the next centres and the history entries;
//   kmeans_label_kernel   the final pass and predict: labels by caller row, counts and inertia under the given centres.
// Centres are broadcast from LDS.  A lane keeps KM_PTS points and their labels in registers; clusters go by in chunks whose masked
// accumulators (label == k ? x : 0) stay in registers, so the order of every sum is fixed.
// Sums: per lane over its points in order, wave totals on the DPP network, a fixed tree over the block's four waves, one slab per block
// in ctx->d_partials, and the last block adds the slabs in a fixed order.  Counts are integers all the way (a slab's count slots hold
// 64-bit integers).  No floating-point atomics, the block count depends on n alone: two runs give the same bits.  Loop state lives on
// the device; passes enqueued behind a stop are no-ops, and the host reads a 40-byte head once per KM_ITERS_PER_SYNC iterations.
#include <cmath>
#include <cstring>
#include <vector>
#include "pcr_internal.h"
#include "pcr_stream_fit.h"
#include "pcr_wave.h"

namespace {

constexpr int KM_MAX_K = PCR_KMEANS_MAX_K;
constexpr int KM_BLOCK = PCR_STREAM_BLOCK;
constexpr int KM_PTS = 4;                        // points per lane, in registers while the clusters go by
constexpr int KM_TILE = KM_PTS * KM_BLOCK;       // points per block: the block count is ceil(n / KM_TILE)
constexpr int KM_CHUNK = 8;                      // clusters per chunk: 8 x dim sums and 8 counts per lane
constexpr int KM_NSUM_MAX = KM_MAX_K * 4 + 1;    // values per block slab: K * (1 + dim) + 1
constexpr int KM_ITERS_PER_SYNC = 8;             // iterations enqueued per read-back of the loop state's head

// Loop state on the device.  The head (the first 40 bytes) is what the host reads per chunk of iterations.
struct __attribute__((aligned(16))) km_state {
    int it;              // completed iterations
    int stop;            // no further assign pass may run
    int converged;       // stopped by shift <= tol
    int n_empty;         // clusters without points in the last pass that counted
    int max_iter, pad;
    double inertia;      // of the centres the last pass assigned under
    double shift;        // max_k |c_new[k] - c_old[k]| of the last update
    double tol;
    double c[KM_MAX_K * 3];        // current centres
    double sums[KM_MAX_K * 3];     // S_k of the last assign pass
    long long counts[KM_MAX_K];    // N_k of the last pass
};
constexpr size_t KM_HEAD_BYTES = offsetof(km_state, tol);
static_assert(KM_HEAD_BYTES == 40, "head of the loop state");
static_assert(sizeof(km_state) <= PCR_SMALL_D2H_BYTES && sizeof(km_state) % 8 == 0, "state read back through pcr_d2h_small");

// squared distance in the direct form, the order of np.sum over (dx^2, dy^2, dz^2)
template <int DIM>
__device__ inline double km_d2(const double* c, double x, double y, double z) {
    const double dx = x - c[0], dy = y - c[1];
    double d = dx * dx + dy * dy;
    if (DIM == 3) { const double dz = z - c[2]; d = d + dz * dz; }
    return d;
}

// block_slab_sums (pcr_wave.h) with integer adds in the count slots (t < K * nt with t % nt == 0), binary64 adds elsewhere
__device__ inline bool km_block_sums(const double (*s_part)[KM_NSUM_MAX], int nsum, int K, int nt, double* __restrict__ partials,
                                     unsigned int* __restrict__ ticket, double (*s_red)[KM_NSUM_MAX], double* s_tot) {
    return block_slab_sums<KM_NSUM_MAX>(s_part, nsum, partials, ticket, s_red, s_tot, [K, nt](double x, double y, int t) {
        const bool count = t < K * nt && t % nt == 0;
        return count ? __longlong_as_double(__double_as_longlong(x) + __double_as_longlong(y)) : x + y;
    });
}

// The block's tile under the centres of `st`: labels (by caller row, if asked for), and per wave in s_part the cluster values
// (SUMS: N_k, S_k at [k * (1 + DIM), ...); else N_k at [k]) and the inertia behind them.
template <int DIM, bool SUMS>
__device__ inline void km_tile_pass(const pcr_pt* __restrict__ pts, long long n, int K, const km_state* __restrict__ st, int* __restrict__ labels,
                                    double* s_c, double (*s_part)[KM_NSUM_MAX]) {
    constexpr int NT = SUMS ? 1 + DIM : 1;
    for (int t = threadIdx.x; t < K * 3; t += KM_BLOCK) s_c[t] = st->c[t];
    double x[KM_PTS], y[KM_PTS], z[KM_PTS];
    int lab[KM_PTS];
    long long id[KM_PTS];
    bool valid[KM_PTS];
    block_tile_load<KM_PTS, true>(pts, n, x, y, z, valid, id);
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double inertia = 0.0;
#pragma unroll
    for (int p = 0; p < KM_PTS; ++p) {
        double best = km_d2<DIM>(s_c, x[p], y[p], z[p]);
        int arg = 0;
        for (int k = 1; k < K; ++k) {
            const double d = km_d2<DIM>(s_c + 3 * k, x[p], y[p], z[p]);
            if (d < best) { best = d; arg = k; }
        }
        lab[p] = valid[p] ? arg : -1;
        inertia += valid[p] ? best : 0.0;
        if (valid[p] && labels) labels[id[p]] = arg;
    }
    inertia = wave_total_f64(inertia);
    if (lane == 63) s_part[wave][K * NT] = inertia;
    for (int k0 = 0; k0 < K; k0 += KM_CHUNK) {
        double acc[KM_CHUNK][3];
        unsigned int cnt[KM_CHUNK];
#pragma unroll
        for (int j = 0; j < KM_CHUNK; ++j) { acc[j][0] = acc[j][1] = acc[j][2] = 0.0; cnt[j] = 0u; }
#pragma unroll
        for (int p = 0; p < KM_PTS; ++p) {
#pragma unroll
            for (int j = 0; j < KM_CHUNK; ++j) {
                const bool mine = lab[p] == k0 + j;
                cnt[j] += mine ? 1u : 0u;
                if (SUMS) {
                    acc[j][0] += mine ? x[p] : 0.0;
                    acc[j][1] += mine ? y[p] : 0.0;
                    if (DIM == 3) acc[j][2] += mine ? z[p] : 0.0;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < KM_CHUNK; ++j) {
            const unsigned int c = wave_incl_scan_add(cnt[j]);   // total in lane 63; every lane takes part
            if (lane == 63 && k0 + j < K) s_part[wave][(k0 + j) * NT] = __longlong_as_double((long long)c);
            if (SUMS) {
#pragma unroll
                for (int d = 0; d < DIM; ++d) {
                    const double v = wave_total_f64(acc[j][d]);
                    if (lane == 63 && k0 + j < K) s_part[wave][(k0 + j) * NT + 1 + d] = v;
                }
            }
        }
    }
}

// One Lloyd iteration.  Slab layout: cluster k at [k * (1 + DIM), ...) = N_k (integer), S_k; the inertia at K * (1 + DIM).
template <int DIM>
__global__ void __launch_bounds__(KM_BLOCK)
kmeans_assign_kernel(const pcr_pt* __restrict__ pts, long long n, int K, km_state* __restrict__ st, double* __restrict__ partials,
                     unsigned int* __restrict__ ticket, double* __restrict__ inertia_hist, double* __restrict__ shift_hist) {
    constexpr int NT = 1 + DIM;
    __shared__ double s_c[KM_MAX_K * 3];
    __shared__ double s_part[4][KM_NSUM_MAX], s_red[8][KM_NSUM_MAX], s_tot[KM_NSUM_MAX];
    if (st->stop) return;
    km_tile_pass<DIM, true>(pts, n, K, st, nullptr, s_c, s_part);
    if (!km_block_sums(s_part, K * NT + 1, K, NT, partials, ticket, s_red, s_tot)) return;

    // ---- the last block: the new centres (an empty cluster keeps its own), the shift, the stop rule
    __shared__ double s_shift[KM_MAX_K];
    __shared__ int s_empty[KM_MAX_K];
    const int k = threadIdx.x;
    if (k < K) {
        const long long nk = __double_as_longlong(s_tot[k * NT]);
        double cn[3] = {s_c[3 * k], s_c[3 * k + 1], s_c[3 * k + 2]};
        if (nk > 0) {
#pragma unroll
            for (int d = 0; d < DIM; ++d) cn[d] = s_tot[k * NT + 1 + d] / (double)nk;
        }
        const double dx = cn[0] - s_c[3 * k], dy = cn[1] - s_c[3 * k + 1];
        double q = dx * dx + dy * dy;
        if (DIM == 3) { const double dz = cn[2] - s_c[3 * k + 2]; q = q + dz * dz; }
        s_shift[k] = sqrt(q);
        s_empty[k] = nk > 0 ? 0 : 1;
        st->counts[k] = nk;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            st->sums[3 * k + d] = d < DIM ? s_tot[k * NT + 1 + d] : 0.0;
            st->c[3 * k + d] = cn[d];
        }
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double shift = 0.0;
    int n_empty = 0;
    for (int j = 0; j < K; ++j) { shift = s_shift[j] > shift ? s_shift[j] : shift; n_empty += s_empty[j]; }
    const int it = st->it;
    const double inertia = s_tot[K * NT];
    if (inertia_hist) inertia_hist[it] = inertia;
    if (shift_hist) shift_hist[it] = shift;
    st->inertia = inertia;
    st->shift = shift;
    st->n_empty = n_empty;
    st->it = it + 1;
    if (shift <= st->tol) { st->converged = 1; st->stop = 1; }
    else if (it + 1 >= st->max_iter) st->stop = 1;
}

// The final pass and predict: labels by CALLER row (the records may be Morton-reordered: id is the row) or none, the counts and the
// inertia under the centres of `st`.  Slab layout: N_k at [k], the inertia at [K].
template <int DIM>
__global__ void __launch_bounds__(KM_BLOCK)
kmeans_label_kernel(const pcr_pt* __restrict__ pts, long long n, int K, km_state* __restrict__ st, double* __restrict__ partials, unsigned int* __restrict__ ticket,
                    int* __restrict__ labels) {
    __shared__ double s_c[KM_MAX_K * 3];
    __shared__ double s_part[4][KM_NSUM_MAX], s_red[8][KM_NSUM_MAX], s_tot[KM_NSUM_MAX];
    km_tile_pass<DIM, false>(pts, n, K, st, labels, s_c, s_part);
    if (!km_block_sums(s_part, K + 1, K, 1, partials, ticket, s_red, s_tot)) return;
    if (threadIdx.x != 0) return;
    int n_empty = 0;
    for (int j = 0; j < K; ++j) {
        const long long nk = __double_as_longlong(s_tot[j]);
        st->counts[j] = nk;
        n_empty += nk > 0 ? 0 : 1;
    }
    st->n_empty = n_empty;
    st->inertia = s_tot[K];
}

bool shape_ok(int k, int dim) { return k >= 1 && k <= KM_MAX_K && (dim == 2 || dim == 3); }
bool all_finite(const double* v, int n) {
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}

void state_from_host(km_state* h, int k, int dim, const double* centers, int max_iter, double tol) {
    memset(h, 0, sizeof(*h));
    h->max_iter = max_iter;
    h->tol = tol;
    for (int j = 0; j < k; ++j)
        for (int c = 0; c < dim; ++c) h->c[3 * j + c] = centers[j * dim + c];
}
void centers_to_host(const double* c3, int k, int dim, double* out) {
    for (int j = 0; j < k; ++j)
        for (int c = 0; c < dim; ++c) out[j * dim + c] = c3[3 * j + c];
}

int km_begin(pcr_stream_fit* r, const pcr_cloud* cloud, int k, int dim, const km_state* h) {
    return pcr_stream_begin(r, cloud, k, dim, KM_TILE, PCR_CW_KMEANS_TICKET, h, sizeof(km_state), KM_NSUM_MAX);
}
int km_assign(pcr_stream_fit* r, double* d_inertia_hist, double* d_shift_hist) {
    return pcr_stream_launch(r, kmeans_assign_kernel<2>, kmeans_assign_kernel<3>, d_inertia_hist, d_shift_hist);
}
int km_label(pcr_stream_fit* r, int* d_labels) { return pcr_stream_launch(r, kmeans_label_kernel<2>, kmeans_label_kernel<3>, d_labels); }

}  // namespace

extern "C" {

void pcr_kmeans_default_params(pcr_kmeans_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->n_clusters = 2;
    p->dim = 3;
    p->max_iter = 300;
    p->tol = 1e-4;
}

int pcr_kmeans_step(pcr_ctx* ctx, const pcr_cloud* cloud, int k, int dim, const double* centers, double* centers_out, int64_t* counts_out, double* sums_out,
                    double* inertia_out, double* shift_out) {
    if (!ctx || !cloud || !centers || !shape_ok(k, dim) || !all_finite(centers, k * dim)) return PCR_E_INVALID;
    if (cloud->n <= 0) return PCR_E_EMPTY;
    hipSetDevice(ctx->device);
    std::vector<km_state> h(1);
    state_from_host(&h[0], k, dim, centers, 1, 0.0);
    pcr_stream_fit r(ctx);
    int rc;
    if ((rc = km_begin(&r, cloud, k, dim, &h[0])) || (rc = km_assign(&r, nullptr, nullptr))) return rc;
    if ((rc = pcr_d2h_small(ctx, &h[0], r.st.p, sizeof(km_state)))) return rc;
    if (centers_out) centers_to_host(h[0].c, k, dim, centers_out);
    if (sums_out) centers_to_host(h[0].sums, k, dim, sums_out);
    if (counts_out) for (int j = 0; j < k; ++j) counts_out[j] = h[0].counts[j];
    if (inertia_out) *inertia_out = h[0].inertia;
    if (shift_out) *shift_out = h[0].shift;
    return PCR_OK;
}

int pcr_kmeans_fit(pcr_ctx* ctx, const pcr_cloud* cloud, const pcr_kmeans_params* params, const double* centers0, double* centers_out, int64_t* counts_out,
                   int32_t* labels_out, double* inertia_hist_out, double* shift_hist_out, pcr_kmeans_result* result) {
    if (!ctx || !cloud || !params || !centers0 || !centers_out || !counts_out || !result) return PCR_E_INVALID;
    const int k = params->n_clusters, dim = params->dim, max_iter = params->max_iter;
    if (!shape_ok(k, dim) || max_iter < 1 || !(params->tol >= 0.0) || !std::isfinite(params->tol) || !all_finite(centers0, k * dim)) return PCR_E_INVALID;
    const int64_t n = cloud->n;
    if (n <= 0) return PCR_E_EMPTY;
    hipSetDevice(ctx->device);
    memset(result, 0, sizeof(*result));
    std::vector<km_state> h(1);
    state_from_host(&h[0], k, dim, centers0, max_iter, params->tol);
    pcr_stream_fit r(ctx);
    pcr_dev_block d_hist(ctx), d_labels(ctx);
    int rc;
    if ((rc = d_hist.alloc(sizeof(double) * 2 * max_iter)) || (labels_out && (rc = d_labels.alloc(sizeof(int32_t) * n)))) return rc;
    double* const d_inertia_hist = d_hist.as<double>();
    double* const d_shift_hist = d_inertia_hist + max_iter;
    PCR_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    if ((rc = km_begin(&r, cloud, k, dim, &h[0]))) return rc;
    // one pass per iteration; passes behind a stop return at once.  Then the final pass under the final centres.
    if ((rc = pcr_stream_loop(&r, max_iter, KM_ITERS_PER_SYNC, KM_HEAD_BYTES, [&](int) { return km_assign(&r, d_inertia_hist, d_shift_hist); }))) return rc;
    if ((rc = km_label(&r, d_labels.as<int>()))) return rc;
    PCR_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    if ((rc = pcr_d2h_small(ctx, &h[0], r.st.p, sizeof(km_state)))) return rc;
    result->iters = h[0].it;
    result->converged = h[0].converged;
    result->n_empty = h[0].n_empty;
    result->inertia = h[0].inertia;
    result->shift = h[0].shift;
    centers_to_host(h[0].c, k, dim, centers_out);
    for (int j = 0; j < k; ++j) counts_out[j] = h[0].counts[j];
    if (inertia_hist_out) PCR_HIP(ctx, hipMemcpyAsync(inertia_hist_out, d_inertia_hist, sizeof(double) * h[0].it, hipMemcpyDeviceToHost, ctx->stream));
    if (shift_hist_out) PCR_HIP(ctx, hipMemcpyAsync(shift_hist_out, d_shift_hist, sizeof(double) * h[0].it, hipMemcpyDeviceToHost, ctx->stream));
    if (inertia_hist_out || shift_hist_out) PCR_HIP(ctx, pcr_sync(ctx->stream));
    if (labels_out && (rc = pcr_d2h_staged(ctx, labels_out, d_labels.p, sizeof(int32_t) * n))) return rc;
    return pcr_events_ms(ctx, &result->device_ms);
}

int pcr_kmeans_predict(pcr_ctx* ctx, const pcr_cloud* cloud, int k, int dim, const double* centers, int32_t* labels_out, int64_t* counts_out,
                       double* inertia_out) {
    if (!ctx || !cloud || !centers || !labels_out || !shape_ok(k, dim) || !all_finite(centers, k * dim)) return PCR_E_INVALID;
    const int64_t n = cloud->n;
    if (n <= 0) return PCR_E_EMPTY;
    hipSetDevice(ctx->device);
    std::vector<km_state> h(1);
    state_from_host(&h[0], k, dim, centers, 1, 0.0);
    pcr_stream_fit r(ctx);
    pcr_dev_block d_labels(ctx);
    int rc;
    if ((rc = d_labels.alloc(sizeof(int32_t) * n)) || (rc = km_begin(&r, cloud, k, dim, &h[0])) || (rc = km_label(&r, d_labels.as<int>()))) return rc;
    if ((rc = pcr_d2h_small(ctx, &h[0], r.st.p, sizeof(km_state)))) return rc;
    if (counts_out) for (int j = 0; j < k; ++j) counts_out[j] = h[0].counts[j];
    if (inertia_out) *inertia_out = h[0].inertia;
    return pcr_d2h_staged(ctx, labels_out, d_labels.p, sizeof(int32_t) * n);
}

}  // extern "C"
