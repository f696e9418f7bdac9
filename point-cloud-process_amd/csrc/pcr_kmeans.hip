// K-Means clustering (Lloyd's iteration): class K_Means of Cluster_KMeans_GMM/compare_cluster.py:16,105,164-170 on a device-resident
// cloud.  The reference's KMeans.py is not in its tree; the semantics are the ones include/pcr.h states.
//
// One streaming pass over the 32-byte records per iteration: the Lloyd pass of pcr_lloyd.h on a cloud source, KM_PTS points per lane.
//   kmeans_assign_kernel  lloyd_assign; the last block also leaves S_k in the state and the two history entries;
//   kmeans_label_kernel   lloyd_label: the final pass and predict, labels by caller row.
// Passes enqueued behind a stop are no-ops; the host reads the state's 40-byte head once per LLOYD_ITERS_PER_SYNC iterations.
#include <cmath>
#include <cstring>
#include <vector>
#include "pcr_internal.h"
#include "pcr_lloyd.h"
#include "pcr_stream_fit.h"

namespace {

constexpr int KM_MAX_K = PCR_KMEANS_MAX_K;
constexpr int KM_PTS = 4;                        // points per lane, in registers while the clusters go by

// The records of a cloud, dim 2 or 3: tiles of KM_PTS * 256 points, labels by CALLER row (Morton-reordered records: id is the row)
template <int DIM>
struct km_cloud_source {
    using rec = pcr_pt;
    static constexpr int KMAX = KM_MAX_K, CSTRIDE = 3, PTS = KM_PTS, DMAX = DIM;
    static constexpr int CHUNK = 8;                  // clusters per chunk: 8 x dim sums and 8 counts per lane
    static constexpr int NSUM = KM_MAX_K * 4 + 1;    // values per block slab: K * (1 + dim) + 1
    __device__ static constexpr int dims(int) { return DIM; }
    __device__ static void load(const pcr_pt* __restrict__ pts, long long n, int, double (&v)[PTS][DMAX], bool (&valid)[PTS], long long (&row)[PTS]) {
        double x[PTS], y[PTS], z[PTS];
        block_tile_load<PTS, true>(pts, n, x, y, z, valid, row);
#pragma unroll
        for (int p = 0; p < PTS; ++p) { v[p][0] = x[p]; v[p][1] = y[p]; if (DIM == 3) v[p][DIM - 1] = z[p]; }
    }
};
constexpr int KM_TILE = KM_PTS * PCR_STREAM_BLOCK;
constexpr int KM_NSUM_MAX = km_cloud_source<3>::NSUM;

struct km_state : lloyd_state<KM_MAX_K, 3> {
    double sums[KM_MAX_K * 3];     // S_k of the last assign pass
};
static_assert(sizeof(km_state) <= PCR_SMALL_D2H_BYTES && sizeof(km_state) % 8 == 0, "state read back through pcr_d2h_small");

template <int DIM>
__global__ void __launch_bounds__(PCR_STREAM_BLOCK)
kmeans_assign_kernel(const pcr_pt* __restrict__ pts, long long n, int K, km_state* __restrict__ st, double* __restrict__ partials,
                     unsigned int* __restrict__ ticket, double* __restrict__ inertia_hist, double* __restrict__ shift_hist) {
    __shared__ lloyd_lds<km_cloud_source<DIM>> s;
    const auto history = [=](int it, double inertia, double shift) {
        if (inertia_hist) inertia_hist[it] = inertia;
        if (shift_hist) shift_hist[it] = shift;
    };
    if (!lloyd_assign<km_cloud_source<DIM>>(pts, n, DIM, K, st, partials, ticket, s, history)) return;
    const int k = threadIdx.x;
    for (int d = 0; d < 3 && k < K; ++d) st->sums[3 * k + d] = d < DIM ? s.tot[k * (1 + DIM) + 1 + d] : 0.0;
}

template <int DIM>
__global__ void __launch_bounds__(PCR_STREAM_BLOCK)
kmeans_label_kernel(const pcr_pt* __restrict__ pts, long long n, int K, km_state* __restrict__ st, double* __restrict__ partials, unsigned int* __restrict__ ticket,
                    int* __restrict__ labels) {
    __shared__ lloyd_lds<km_cloud_source<DIM>> s;
    lloyd_label<km_cloud_source<DIM>>(pts, n, DIM, K, st, partials, ticket, labels, s);
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
    return pcr_stream_begin(r, cloud->d, cloud->n, k, dim, KM_TILE, PCR_CW_KMEANS_TICKET, h, sizeof(km_state), KM_NSUM_MAX);
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
    if ((rc = pcr_stream_loop(&r, max_iter, LLOYD_ITERS_PER_SYNC, LLOYD_HEAD_BYTES, [&](int) { return km_assign(&r, d_inertia_hist, d_shift_hist); }))) return rc;
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
