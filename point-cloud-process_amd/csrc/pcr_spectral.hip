// Spectral clustering: class spetral_clustering of Cluster_KMeans_GMM/spectral_clustering.py:7-46 on a device-resident cloud.  The
// semantics are the ones include/pcr.h states.
//
//   graph     grid index -> exact k-NN of the cloud's own records (pcr_knn_dev, k = nnk + 1) -> both directions of every edge as
//             (row << 32 | column, 1 / dist) pairs -> radix sort -> group heads drop the second copy of a mutual pair and give the row
//             starts: a CSR with ascending columns.  Rows and columns are positions in the index's Morton order, so a row's neighbours
//             sit near it in memory (pcr_knn_graph and the dense path of small clouds ask for caller rows instead).
//   solver    Chebyshev-filtered subspace iteration on B (spectrum in [-1, 1]) with a block of p = m + 8 binary64 vectors, row-major
//             (n, p): a gathered neighbour row is one piece of 8 p bytes.
//               sp_spmm_kernel    Y2 = alpha B Y1 + beta Y1 + gamma Y0: one step of the three-term recurrence per launch, 16 lanes per row
//               sp_gram_kernel    X^T Y in per-block slabs, summed in block order by the last block (block_slab_sums), which then either
//                                 scales the columns and inverts the Cholesky factor (Cholesky-QR) or runs the Jacobi solve of the
//                                 Rayleigh-Ritz step; the p x p result T is left in the loop state
//               sp_apply_kernel   X <- X T (and Y <- Y T, the residual norms |B u - theta u| and the stop rule)
//             One read-back of the state's head per outer iteration.
//   k-means   the Lloyd pass of pcr_lloyd.h on the rows of the (n, m) embedding, one row per lane; maximin seeds by one block.
// No floating-point atomics; every grid depends on n alone: two runs give the same bits.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>
#include "pcr_internal.h"
#include "pcr_lloyd.h"
#include "pcr_sort.h"
#include "pcr_spectral_dev.h"
#include "pcr_stream_fit.h"
#include "pcr_wave.h"

namespace {

constexpr int SP_MAX_K = PCR_SPECTRAL_MAX_K;
constexpr int SP_GUARD = 8;                      // guard vectors behind the m wanted ones
constexpr int SP_MAX_P = SP_MAX_K + SP_GUARD;    // 16: lanes per row
constexpr int SP_NG = SP_MAX_P * SP_MAX_P;       // slots of a Gram slab (stride 16 whatever p)
constexpr int SP_DEGREE = 20;                    // of the Chebyshev filter
constexpr int SP_DENSE_N = 64;                   // clouds up to this size take the dense path
constexpr int SP_ROWS = 16;                      // rows per block of the product (256 threads)
constexpr int SP_APPLY_ROWS = 64;                // rows per block of sp_apply_kernel
constexpr int SP_GRAM_ROWS = 256;                // rows per block of sp_gram_kernel, staged 64 at a time

// ---------------------------------------------------------------------------------------------------------------- graph
struct sp_graph {
    pcr_dev_block indptr, cols, w, rows;   // unsigned[n + 1], unsigned[nnz], double[nnz]; long long[n]: the caller row of every graph row
    long long n = 0, nnz = 0;
    explicit sp_graph(pcr_ctx* c) : indptr(c), cols(c), w(c), rows(c) {}
};

// the queries of the k-NN = the index's own records, in its order; where every caller row went
__global__ void __launch_bounds__(256)
sp_queries_kernel(const pcr_pt* __restrict__ sorted, long long n, double* __restrict__ q, unsigned int* __restrict__ pos_of_row, long long* __restrict__ rows) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const pcr_pt r = sorted[i];
    q[3 * i] = r.x; q[3 * i + 1] = r.y; q[3 * i + 2] = r.z;
    pos_of_row[r.id] = (unsigned int)i;
    rows[i] = r.id;
}

// both directions of the nnk nearest other rows of record i.  BY_CALLER: rows and columns are caller rows, else positions.
template <bool BY_CALLER>
__global__ void __launch_bounds__(256)
sp_emit_kernel(const long long* __restrict__ rows, long long n, int k, int nnk, const int* __restrict__ idx, const double* __restrict__ dist,
               const unsigned int* __restrict__ pos_of_row, unsigned long long* __restrict__ keys, double* __restrict__ vals, int* __restrict__ bad_row) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long id = rows[i];
    const unsigned long long r = BY_CALLER ? (unsigned long long)id : (unsigned long long)i;
    int cnt = 0;
    for (int j = 0; j < k && cnt < nnk; ++j) {
        const int nb = idx[i * k + j];
        if ((long long)nb == id) continue;   // the row itself, dropped by id
        const double d = dist[i * k + j];
        if (!(d > 0.0)) atomicMin(bad_row, (int)id);
        const double w = 1.0 / d;
        const unsigned long long c = BY_CALLER ? (unsigned long long)nb : (unsigned long long)pos_of_row[nb];
        const long long at = 2 * (i * nnk + cnt);
        keys[at] = (r << 32) | c; vals[at] = w;
        keys[at + 1] = (c << 32) | r; vals[at + 1] = w;
        ++cnt;
    }
}

__global__ void __launch_bounds__(256)
sp_compact_kernel(const unsigned long long* __restrict__ keys, const double* __restrict__ vals, const unsigned int* __restrict__ heads, long long nnz,
                  unsigned int* __restrict__ cols, double* __restrict__ w) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nnz) return;
    const unsigned int h = heads[e];
    cols[e] = (unsigned int)(keys[h] & 0xffffffffull);
    w[e] = vals[h];   // (the two copies of a mutual pair carry the same bits: (a - b)^2 == (b - a)^2)
}

// row starts: the first group head whose key is not below (row << 32)
__global__ void __launch_bounds__(256)
sp_indptr_kernel(const unsigned long long* __restrict__ keys, const unsigned int* __restrict__ heads, long long nnz, long long n, unsigned int* __restrict__ indptr) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n) return;
    const unsigned long long want = (unsigned long long)r << 32;
    long long lo = 0, hi = nnz;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (keys[heads[mid]] < want) lo = mid + 1; else hi = mid;
    }
    indptr[r] = (unsigned int)lo;
}

int sp_build_graph(pcr_ctx* ctx, const pcr_cloud* cloud, int nnk, bool by_caller, sp_graph* g, int* bad_row_out) {
    const long long n = cloud->n;
    const int k = nnk + 1;
    const long long n_pairs = 2 * n * nnk;
    *bad_row_out = -1;
    g->n = n;
    pcr_index_guard index(ctx);
    int rc;
    if ((rc = pcr_index_build(ctx, cloud, PCR_INDEX_GRID, 0.0, &index.h))) return rc;
    pcr_dev_block d_q(ctx), d_pos(ctx), d_idx(ctx), d_dist(ctx), d_keys(ctx), d_keys2(ctx), d_vals(ctx), d_vals2(ctx), d_heads(ctx), d_small(ctx), d_tmp(ctx), d_tmp2(ctx);
    if ((rc = d_q.alloc(sizeof(double) * 3 * n)) || (rc = d_pos.alloc(sizeof(unsigned int) * n)) || (rc = g->rows.alloc(sizeof(long long) * n)) ||
        (rc = d_idx.alloc(sizeof(int) * n * k)) || (rc = d_dist.alloc(sizeof(double) * n * k)) || (rc = d_keys.alloc(8 * n_pairs)) || (rc = d_keys2.alloc(8 * n_pairs)) ||
        (rc = d_vals.alloc(8 * n_pairs)) || (rc = d_vals2.alloc(8 * n_pairs)) || (rc = d_heads.alloc(4 * n_pairs)) || (rc = d_small.alloc(16)))
        return rc;
    const unsigned gn = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(sp_queries_kernel, dim3(gn), dim3(256), 0, ctx->stream, (const pcr_pt*)index->sorted, n, d_q.as<double>(), d_pos.as<unsigned int>(), g->rows.as<long long>());
    PCR_HIP(ctx, hipGetLastError());
    if ((rc = pcr_knn_dev(ctx, index.h, d_q.as<const double>(), n, k, d_idx.as<int>(), d_dist.as<double>()))) return rc;
    unsigned int* d_ngroups = d_small.as<unsigned int>();
    int* d_bad = d_small.as<int>() + 1;
    const int h_init[2] = {0, INT_MAX};
    PCR_HIP(ctx, hipMemcpyAsync(d_small.p, h_init, sizeof(h_init), hipMemcpyHostToDevice, ctx->stream));
    if (by_caller)
        hipLaunchKernelGGL(sp_emit_kernel<true>, dim3(gn), dim3(256), 0, ctx->stream, g->rows.as<const long long>(), n, k, nnk, d_idx.as<const int>(), d_dist.as<const double>(),
                           d_pos.as<const unsigned int>(), d_keys.as<unsigned long long>(), d_vals.as<double>(), d_bad);
    else
        hipLaunchKernelGGL(sp_emit_kernel<false>, dim3(gn), dim3(256), 0, ctx->stream, g->rows.as<const long long>(), n, k, nnk, d_idx.as<const int>(), d_dist.as<const double>(),
                           d_pos.as<const unsigned int>(), d_keys.as<unsigned long long>(), d_vals.as<double>(), d_bad);
    PCR_HIP(ctx, hipGetLastError());
    int row_bits = 1;
    while ((1ll << row_bits) < n) ++row_bits;
    if ((rc = pcr_sort_pairs_arena(ctx, d_keys.as<unsigned long long>(), d_keys2.as<unsigned long long>(), d_vals.as<double>(), d_vals2.as<double>(), (size_t)n_pairs,
                                   (unsigned int)(32 + row_bits), d_tmp)))
        return rc;
    if ((rc = pcr_group_heads(ctx, d_keys2.as<const unsigned long long>(), (size_t)n_pairs, d_heads.as<unsigned int>(), d_ngroups, d_tmp2))) return rc;
    int h_small[2] = {0, 0};
    if ((rc = pcr_d2h_small(ctx, h_small, d_small.p, sizeof(h_small)))) return rc;
    if (h_small[1] != INT_MAX) { *bad_row_out = h_small[1]; return PCR_E_SINGULAR; }
    const long long nnz = (unsigned int)h_small[0];
    g->nnz = nnz;
    if ((rc = g->indptr.alloc(sizeof(unsigned int) * (n + 1))) || (rc = g->cols.alloc(sizeof(unsigned int) * nnz)) || (rc = g->w.alloc(sizeof(double) * nnz))) return rc;
    hipLaunchKernelGGL(sp_compact_kernel, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, ctx->stream, d_keys2.as<const unsigned long long>(), d_vals2.as<const double>(),
                       d_heads.as<const unsigned int>(), nnz, g->cols.as<unsigned int>(), g->w.as<double>());
    hipLaunchKernelGGL(sp_indptr_kernel, dim3((unsigned)((n + 256) / 256)), dim3(256), 0, ctx->stream, d_keys2.as<const unsigned long long>(), d_heads.as<const unsigned int>(), nnz, n,
                       g->indptr.as<unsigned int>());
    PCR_HIP(ctx, hipGetLastError());
    PCR_HIP(ctx, pcr_sync(ctx->stream));   // the scratch above goes back to the arena behind the last kernel that reads it
    return PCR_OK;
}

// ---------------------------------------------------------------------------------------------------------------- solver
// Loop state on the device; the host reads the head once per outer iteration.
struct __attribute__((aligned(16))) sp_state {
    int fail;                      // a Cholesky pivot (or a column norm) was not positive or not finite
    int converged;                 // r_j <= 2 tol for all j < m
    int max_degree, pad;
    unsigned long long dmax_bits;  // the largest degree (bits of a positive binary64 order like integers)
    double min_pivot;              // the smallest Cholesky pivot of the last factorisation (unit diagonal)
    double theta[SP_MAX_P], resid[SP_MAX_P];
    double scale[SP_MAX_K];        // per embedding column: sign / norm
    double T[SP_NG];               // the p x p matrix the next sp_apply_kernel multiplies by (stride 16)
};
constexpr size_t SP_HEAD_BYTES = offsetof(sp_state, scale);
static_assert(sizeof(sp_state) <= PCR_SMALL_D2H_BYTES, "state read back through pcr_d2h_small");

// degrees in column order, the largest degree and the longest row
__global__ void __launch_bounds__(256)
sp_degree_kernel(const unsigned int* __restrict__ indptr, const double* __restrict__ w, long long n, double* __restrict__ deg, sp_state* __restrict__ st) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned int s = indptr[i], e = indptr[i + 1];
    double d = 0.0;
    for (unsigned int j = s; j < e; ++j) d += w[j];
    deg[i] = d;
    atomicMax(&st->dmax_bits, (unsigned long long)__double_as_longlong(d));
    atomicMax(&st->max_degree, (int)(e - s));
}

// the operator's entries: normalized w (s_i s_j) with s = d^-1/2 and a zero diagonal; else w / d_max and 1 - d_i / d_max.  Both are
// symmetric to the bit.
__global__ void __launch_bounds__(256)
sp_operator_kernel(const unsigned int* __restrict__ indptr, const unsigned int* __restrict__ cols, const double* __restrict__ w, const double* __restrict__ deg, long long n,
                   int normalized, const sp_state* __restrict__ st, double* __restrict__ bval, double* __restrict__ diag) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double dmax = __longlong_as_double((long long)st->dmax_bits);
    const double si = 1.0 / sqrt(deg[i]);
    for (unsigned int j = indptr[i]; j < indptr[i + 1]; ++j) bval[j] = normalized ? w[j] * (si * (1.0 / sqrt(deg[cols[j]]))) : w[j] / dmax;
    diag[i] = normalized ? 0.0 : 1.0 - deg[i] / dmax;
}

__global__ void __launch_bounds__(256)
sp_start_kernel(const long long* __restrict__ rows, long long n, int p, double* __restrict__ X) {
    const long long i = (long long)blockIdx.x * SP_ROWS + (threadIdx.x >> 4);
    const int c = threadIdx.x & 15;
    if (i < n && c < p) X[i * p + c] = pcr_spectral_start(rows[i], c);
}

// Y2 = alpha (B Y1) + beta Y1 + gamma Y0 (Y0 null: no third term).  16 lanes per row, lane c owns column c: a gathered row is one
// contiguous read of 8 p bytes, the edge's column and value are broadcast loads.
__global__ void __launch_bounds__(256)
sp_spmm_kernel(const unsigned int* __restrict__ indptr, const unsigned int* __restrict__ cols, const double* __restrict__ bval, const double* __restrict__ diag, long long n, int p,
               const double* __restrict__ Y1, const double* __restrict__ Y0, double* __restrict__ Y2, double alpha, double beta, double gamma) {
    const long long i = (long long)blockIdx.x * SP_ROWS + (threadIdx.x >> 4);
    const int c = threadIdx.x & 15;
    if (i >= n || c >= p) return;
    const double own = Y1[i * p + c];
    double acc = diag[i] * own;
    const unsigned int e1 = indptr[i + 1];
    for (unsigned int e = indptr[i]; e < e1; ++e) acc += bval[e] * Y1[(long long)cols[e] * p + c];
    double v = alpha * acc + beta * own;
    if (Y0) v += gamma * Y0[i * p + c];
    Y2[i * p + c] = v;
}

// X^T Y (p x p).  RITZ = false: X = Y; the last block scales to a unit diagonal, factors G = R^T R and leaves T = D^-1 R^-1, so that
// X T has orthonormal columns (one step of Cholesky-QR, with the column scaling in front).  RITZ = true: Y = B X; the last block
// symmetrises H = X^T Y, solves it by Jacobi and leaves T = its eigenvectors by descending eigenvalue, theta = the eigenvalues.
template <bool RITZ>
__global__ void __launch_bounds__(256)
sp_gram_kernel(const double* __restrict__ X, const double* __restrict__ Y, long long n, int p, sp_state* __restrict__ st, double* __restrict__ partials,
               unsigned int* __restrict__ ticket) {
    __shared__ double s_x[64 * SP_MAX_P], s_y[64 * SP_MAX_P];
    __shared__ double s_part[4][SP_NG], s_red[8][SP_NG], s_tot[SP_NG];
    const int a = threadIdx.x >> 4, b = threadIdx.x & 15;
    const bool live = a < p && b < p;
    const long long total = n * p;
    double acc = 0.0;
    for (int chunk = 0; chunk < SP_GRAM_ROWS / 64; ++chunk) {
        const long long base = ((long long)blockIdx.x * SP_GRAM_ROWS + chunk * 64) * p;
        __syncthreads();
        for (int t = threadIdx.x; t < 64 * p; t += 256) {
            const bool in = base + t < total;
            s_x[t] = in ? X[base + t] : 0.0;
            if (RITZ) s_y[t] = in ? Y[base + t] : 0.0;
        }
        __syncthreads();
        if (live) {
            const double* sy = RITZ ? s_y : s_x;
            for (int r = 0; r < 64; ++r) acc += s_x[r * p + a] * sy[r * p + b];
        }
    }
    s_part[0][threadIdx.x] = live ? acc : 0.0;
    s_part[1][threadIdx.x] = s_part[2][threadIdx.x] = s_part[3][threadIdx.x] = 0.0;
    if (!block_slab_sums<SP_NG>(s_part, SP_NG, partials, ticket, s_red, s_tot, [](double x, double y, int) { return x + y; })) return;

    // ---- the last block
    __shared__ double s_A[SP_NG], s_V[SP_NG];
    if (RITZ) {
        if (live) s_A[a * p + b] = 0.5 * (s_tot[a * SP_MAX_P + b] + s_tot[b * SP_MAX_P + a]);
        __syncthreads();
        if (threadIdx.x < 64) pcr_jacobi_eig(p, s_A, s_V, (int)threadIdx.x, 64, [] { wave_sync(); });
        __syncthreads();
        if (threadIdx.x == 0) {
            int order[SP_MAX_P];
            pcr_order_desc(p, s_A, order);
            for (int j = 0; j < p; ++j) {
                st->theta[j] = s_A[order[j] * p + order[j]];
                for (int i = 0; i < p; ++i) st->T[i * SP_MAX_P + j] = s_V[i * p + order[j]];
            }
        }
        return;
    }
    if (threadIdx.x != 0) return;
    double nrm[SP_MAX_P];
    bool ok = true;
    for (int i = 0; i < p; ++i) {
        const double g = s_tot[i * SP_MAX_P + i];
        nrm[i] = sqrt(g);
        ok = ok && g > 0.0 && isfinite(g);
    }
    double min_piv = 1.0;
    // s_A = R (upper), s_V = R^-1 (upper), stride p
    for (int j = 0; j < p && ok; ++j) {
        for (int i = 0; i <= j; ++i) {
            double sum = s_tot[i * SP_MAX_P + j] / (nrm[i] * nrm[j]);
            for (int k = 0; k < i; ++k) sum -= s_A[k * p + i] * s_A[k * p + j];
            if (i == j) {
                if (!(sum > 0.0) || !isfinite(sum)) { ok = false; break; }
                min_piv = sum < min_piv ? sum : min_piv;
                s_A[j * p + j] = sqrt(sum);
            } else {
                s_A[i * p + j] = sum / s_A[i * p + i];
            }
        }
    }
    if (!ok) { st->fail = 1; return; }
    for (int j = 0; j < p; ++j) {   // column j of R^-1 by back substitution: R x = e_j
        for (int i = p - 1; i >= 0; --i) {
            if (i > j) { s_V[i * p + j] = 0.0; continue; }
            double sum = i == j ? 1.0 : 0.0;
            for (int k = i + 1; k <= j; ++k) sum -= s_A[i * p + k] * s_V[k * p + j];
            s_V[i * p + j] = sum / s_A[i * p + i];
        }
    }
    for (int i = 0; i < p; ++i)
        for (int j = 0; j < p; ++j) st->T[i * SP_MAX_P + j] = s_V[i * p + j] / nrm[i];
    st->min_pivot = min_piv;
}

// X <- X T.  RESID: also Y <- Y T (Y = B X before, B U after), the column sums of (B u - theta u)^2 in per-block slabs; the last
// block leaves the residual norms and the stop rule in the state.
template <bool RESID>
__global__ void __launch_bounds__(256)
sp_apply_kernel(double* __restrict__ X, double* __restrict__ Y, long long n, int p, int m, double tol2, sp_state* __restrict__ st, double* __restrict__ partials,
                unsigned int* __restrict__ ticket) {
    __shared__ double s_T[SP_NG], s_theta[SP_MAX_P];
    __shared__ double s_x[SP_APPLY_ROWS / 16][256], s_y[SP_APPLY_ROWS / 16][256];
    __shared__ double s_part[4][SP_MAX_P], s_red[8][SP_MAX_P], s_tot[SP_MAX_P];
    const int g = threadIdx.x >> 4, c = threadIdx.x & 15;
    s_T[threadIdx.x] = (g < p && c < p) ? st->T[threadIdx.x] : 0.0;
    if (threadIdx.x < SP_MAX_P) s_theta[threadIdx.x] = threadIdx.x < (unsigned)p ? st->theta[threadIdx.x] : 0.0;
    for (int it = 0; it < SP_APPLY_ROWS / 16; ++it) {
        const long long row = (long long)blockIdx.x * SP_APPLY_ROWS + it * 16 + g;
        const bool in = row < n && c < p;
        s_x[it][threadIdx.x] = in ? X[row * p + c] : 0.0;
        if (RESID) s_y[it][threadIdx.x] = in ? Y[row * p + c] : 0.0;
    }
    __syncthreads();
    double sq = 0.0;
    for (int it = 0; it < SP_APPLY_ROWS / 16; ++it) {
        const long long row = (long long)blockIdx.x * SP_APPLY_ROWS + it * 16 + g;
        const bool in = row < n && c < p;
        double u = 0.0, bu = 0.0;
        for (int a = 0; a < p; ++a) {
            u += s_x[it][g * 16 + a] * s_T[a * SP_MAX_P + c];
            if (RESID) bu += s_y[it][g * 16 + a] * s_T[a * SP_MAX_P + c];
        }
        if (in) X[row * p + c] = u;
        if (RESID) {
            if (in) Y[row * p + c] = bu;
            const double r = bu - s_theta[c] * u;
            sq += in ? r * r : 0.0;
        }
    }
    if (!RESID) return;
    // column sums over the block's 16 row groups, in group order
    __syncthreads();
    s_x[0][threadIdx.x] = sq;
    __syncthreads();
    if (threadIdx.x < SP_MAX_P) {
        double v = 0.0;
        for (int gg = 0; gg < 16; ++gg) v += s_x[0][gg * 16 + threadIdx.x];
        s_part[0][threadIdx.x] = v;
        s_part[1][threadIdx.x] = s_part[2][threadIdx.x] = s_part[3][threadIdx.x] = 0.0;
    }
    if (!block_slab_sums<SP_MAX_P>(s_part, SP_MAX_P, partials, ticket, s_red, s_tot, [](double x, double y, int) { return x + y; })) return;
    if (threadIdx.x != 0) return;
    int conv = 1;
    for (int j = 0; j < p; ++j) {
        const double r = sqrt(s_tot[j]);
        st->resid[j] = r;
        if (j < m && !(r <= tol2)) conv = 0;
    }
    st->converged = conv;
}

// ---------------------------------------------------------------------------------------------------------------- embedding
// E[caller row][j] = u_j (not normalized) or d^-1/2 u_j, j < m
__global__ void __launch_bounds__(256)
sp_embed_kernel(const double* __restrict__ U, const double* __restrict__ deg, const long long* __restrict__ rows, long long n, int p, int m, int normalized,
                double* __restrict__ E) {
    const long long i = (long long)blockIdx.x * SP_ROWS + (threadIdx.x >> 4);
    const int c = threadIdx.x & 15;
    if (i >= n || c >= m) return;
    const double u = U[i * p + c];
    E[rows[i] * m + c] = normalized ? u / sqrt(deg[i]) : u;
}

// thread 0's pick among the block's 256 candidates (a thread without rows holds row -1): the largest value, the lowest row on ties
__device__ inline long long sp_pick_row(const double* s_val, const long long* s_row) {
    double b = -1.0;
    long long br = -1;
    for (int t = 0; t < 256; ++t)
        if (s_row[t] >= 0 && (s_val[t] > b || (s_val[t] == b && s_row[t] < br))) { b = s_val[t]; br = s_row[t]; }
    return br;
}

// ONE block: per column the 2-norm (thread t sums the rows t, t + 256, ... in order, thread 0 the 256 partial sums in order) and the
// entry of largest magnitude, the lowest row on ties -> scale[j] = +-1 / norm
__global__ void __launch_bounds__(256)
sp_colscale_kernel(const double* __restrict__ E, long long n, int m, double* __restrict__ scale) {
    __shared__ double s_sum[256], s_abs[256];
    __shared__ long long s_row[256];
    for (int j = 0; j < m; ++j) {
        double sum = 0.0, best = -1.0;
        long long brow = -1;
        for (long long i = threadIdx.x; i < n; i += 256) {
            const double v = E[i * m + j];
            sum += v * v;
            if (fabs(v) > best) { best = fabs(v); brow = i; }
        }
        s_sum[threadIdx.x] = sum; s_abs[threadIdx.x] = best; s_row[threadIdx.x] = brow;
        __syncthreads();
        if (threadIdx.x == 0) {
            double tot = 0.0;
            for (int t = 0; t < 256; ++t) tot += s_sum[t];
            const long long br = sp_pick_row(s_abs, s_row);
            const double sign = (br >= 0 && E[br * m + j] < 0.0) ? -1.0 : 1.0;
            scale[j] = sign / sqrt(tot);
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256)
sp_scale_kernel(double* __restrict__ E, long long n, int m, const double* __restrict__ scale) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n * m) E[t] = E[t] * scale[t % m];
}

// ---------------------------------------------------------------------------------------------------------------- k-means on rows
// The rows of an (n, m) matrix, m <= SP_MAX_K at run time: one row per lane, labels by row
struct sp_row_source {
    using rec = double;
    static constexpr int KMAX = SP_MAX_K, CSTRIDE = SP_MAX_K, PTS = 1, DMAX = SP_MAX_K, CHUNK = 1;
    static constexpr int NSUM = SP_MAX_K * (1 + SP_MAX_K) + 1;
    __device__ static int dims(int m) { return m; }
    __device__ static void load(const double* __restrict__ E, long long n, int m, double (&x)[1][DMAX], bool (&valid)[1], long long (&row)[1]) {
        const long long i = (long long)blockIdx.x * PCR_STREAM_BLOCK + threadIdx.x;
        valid[0] = i < n;
        row[0] = i;
#pragma unroll
        for (int d = 0; d < DMAX; ++d) x[0][d] = (valid[0] && d < m) ? E[i * m + d] : 0.0;
    }
};

struct sp_km_state : lloyd_state<SP_MAX_K, SP_MAX_K> {
    long long seeds[SP_MAX_K];
};
static_assert(sizeof(sp_km_state) <= PCR_SMALL_D2H_BYTES, "state read back through pcr_d2h_small");

// maximin seeds by ONE block: seed 0 = row 0; seed j = the row with the largest minimum squared distance to the seeds before it
__global__ void __launch_bounds__(256)
sp_maximin_kernel(const double* __restrict__ E, long long n, int m, int K, double* __restrict__ mind, sp_km_state* __restrict__ st) {
    __shared__ double s_c[SP_MAX_K], s_val[256];
    __shared__ long long s_row[256], s_last;
    if (threadIdx.x == 0) { s_last = 0; st->seeds[0] = 0; }
    __syncthreads();
    for (int j = 1; j < K; ++j) {
        if (threadIdx.x < (unsigned)m) s_c[threadIdx.x] = E[s_last * m + threadIdx.x];
        __syncthreads();
        double best = -1.0;
        long long brow = -1;
        for (long long i = threadIdx.x; i < n; i += 256) {
            double d0 = E[i * m] - s_c[0];
            double d2 = d0 * d0;
            for (int d = 1; d < m; ++d) { const double dd = E[i * m + d] - s_c[d]; d2 = d2 + dd * dd; }
            const double md = j == 1 ? d2 : fmin(mind[i], d2);
            mind[i] = md;
            if (md > best) { best = md; brow = i; }
        }
        s_val[threadIdx.x] = best; s_row[threadIdx.x] = brow;
        __syncthreads();
        if (threadIdx.x == 0) {
            const long long br = sp_pick_row(s_val, s_row);
            s_last = br;
            st->seeds[j] = br;
        }
        __syncthreads();
    }
}

__global__ void sp_km_seed_kernel(const double* __restrict__ E, int m, int K, sp_km_state* __restrict__ st) {
    const int k = threadIdx.x / SP_MAX_K, d = threadIdx.x % SP_MAX_K;
    if (k < K) st->c[k * SP_MAX_K + d] = d < m ? E[st->seeds[k] * m + d] : 0.0;
}

__global__ void __launch_bounds__(PCR_STREAM_BLOCK)
sp_km_assign_kernel(const double* __restrict__ E, long long n, int K, sp_km_state* __restrict__ st, double* __restrict__ partials, unsigned int* __restrict__ ticket, int m) {
    __shared__ lloyd_lds<sp_row_source> s;
    lloyd_assign<sp_row_source>(E, n, m, K, st, partials, ticket, s, [](int, double, double) {});
}

__global__ void __launch_bounds__(PCR_STREAM_BLOCK)
sp_km_label_kernel(const double* __restrict__ E, long long n, int K, sp_km_state* __restrict__ st, double* __restrict__ partials, unsigned int* __restrict__ ticket, int m,
                   int* __restrict__ labels) {
    __shared__ lloyd_lds<sp_row_source> s;
    lloyd_label<sp_row_source>(E, n, m, K, st, partials, ticket, labels, s);
}

// ---------------------------------------------------------------------------------------------------------------- host
bool params_ok(const pcr_spectral_params* p) {
    return p->n_clusters >= 1 && p->n_clusters <= SP_MAX_K && p->nnk >= 1 && p->nnk <= PCR_SPECTRAL_MAX_NNK && p->max_iter >= 1 && p->kmeans_max_iter >= 1 &&
           std::isfinite(p->tol) && p->tol > 0.0 && std::isfinite(p->kmeans_tol) && p->kmeans_tol >= 0.0;
}

// checks that need n: PCR_E_EMPTY, then the cloud's size against nnk and m, then the seed rows
int cloud_ok(const pcr_cloud* cloud, int nnk, int m, const int64_t* seed_rows) {
    const int64_t n = cloud->n;
    if (n <= 0) return PCR_E_EMPTY;
    if (n < nnk + 2 || n < m || n > 0x7fffffffll / (2 * PCR_SPECTRAL_MAX_NNK + 2)) return PCR_E_INVALID;
    if (seed_rows)
        for (int j = 0; j < m; ++j) {
            if (seed_rows[j] < 0 || seed_rows[j] >= n) return PCR_E_INVALID;
            for (int i = 0; i < j; ++i)
                if (seed_rows[i] == seed_rows[j]) return PCR_E_INVALID;
        }
    return PCR_OK;
}

// the dense path of small clouds, on the host: `g` is by caller row.  E (n x m) gets the finished embedding.
int dense_embed(pcr_ctx* ctx, const sp_graph& g, int m, int normalized, std::vector<double>& E, pcr_spectral_result* res) {
    const int n = (int)g.n;
    std::vector<unsigned int> indptr(n + 1), cols((size_t)g.nnz);
    std::vector<double> w((size_t)g.nnz), deg(n), B((size_t)n * n, 0.0), A, V((size_t)n * n);
    PCR_HIP(ctx, hipMemcpyAsync(indptr.data(), g.indptr.p, 4 * (size_t)(n + 1), hipMemcpyDeviceToHost, ctx->stream));
    PCR_HIP(ctx, hipMemcpyAsync(cols.data(), g.cols.p, 4 * (size_t)g.nnz, hipMemcpyDeviceToHost, ctx->stream));
    PCR_HIP(ctx, hipMemcpyAsync(w.data(), g.w.p, 8 * (size_t)g.nnz, hipMemcpyDeviceToHost, ctx->stream));
    PCR_HIP(ctx, pcr_sync(ctx->stream));
    double dmax = 0.0;
    int max_degree = 0;
    for (int i = 0; i < n; ++i) {
        double d = 0.0;
        for (unsigned int e = indptr[i]; e < indptr[i + 1]; ++e) d += w[e];
        deg[i] = d;
        dmax = d > dmax ? d : dmax;
        max_degree = std::max(max_degree, (int)(indptr[i + 1] - indptr[i]));
    }
    for (int i = 0; i < n; ++i) {
        const double si = 1.0 / sqrt(deg[i]);
        for (unsigned int e = indptr[i]; e < indptr[i + 1]; ++e) B[(size_t)i * n + cols[e]] = normalized ? w[e] * (si * (1.0 / sqrt(deg[cols[e]]))) : w[e] / dmax;
        B[(size_t)i * n + i] = normalized ? 0.0 : 1.0 - deg[i] / dmax;
    }
    A = B;
    pcr_jacobi_eig(n, A.data(), V.data(), 0, 1, [] {});
    std::vector<int> order(n);
    pcr_order_desc(n, A.data(), order.data());
    const double scale = normalized ? 1.0 : dmax;
    res->max_degree = max_degree;
    res->converged = 1;
    res->next_eigenvalue = m < n ? scale * (1.0 - A[(size_t)order[m] * n + order[m]]) : NAN;
    E.assign((size_t)n * m, 0.0);
    for (int j = 0; j < m; ++j) {
        const int o = order[j];
        const double theta = A[(size_t)o * n + o];
        res->eigenvalues[j] = scale * (1.0 - theta);
        double r2 = 0.0;
        for (int i = 0; i < n; ++i) {
            double bu = 0.0;
            for (int c = 0; c < n; ++c) bu += B[(size_t)i * n + c] * V[(size_t)c * n + o];
            const double r = bu - theta * V[(size_t)i * n + o];
            r2 += r * r;
        }
        res->residuals[j] = sqrt(r2);
        double sum = 0.0, best = -1.0;
        int brow = 0;
        for (int i = 0; i < n; ++i) {
            const double v = normalized ? V[(size_t)i * n + o] / sqrt(deg[i]) : V[(size_t)i * n + o];
            E[(size_t)i * m + j] = v;
            sum += v * v;
            if (fabs(v) > best) { best = fabs(v); brow = i; }
        }
        const double s = (E[(size_t)brow * m + j] < 0.0 ? -1.0 : 1.0) / sqrt(sum);
        for (int i = 0; i < n; ++i) E[(size_t)i * m + j] = E[(size_t)i * m + j] * s;
    }
    return PCR_OK;
}

// the subspace iteration on the device: `g` is in the index's order.  d_E (n x m, by caller row) gets the finished embedding.
int device_embed(pcr_ctx* ctx, const sp_graph& g, const pcr_spectral_params* params, double* d_E, pcr_spectral_result* res) {
    const long long n = g.n;
    const int m = params->n_clusters, p = m + SP_GUARD, normalized = params->normalized ? 1 : 0;
    const double tol2 = 2.0 * params->tol;
    pcr_dev_block b_buf[3] = {pcr_dev_block(ctx), pcr_dev_block(ctx), pcr_dev_block(ctx)};
    pcr_dev_block b_deg(ctx), b_bval(ctx), b_diag(ctx), b_st(ctx);
    int rc;
    for (int i = 0; i < 3; ++i)
        if ((rc = b_buf[i].alloc(sizeof(double) * n * p))) return rc;
    if ((rc = b_deg.alloc(8 * n)) || (rc = b_bval.alloc(8 * g.nnz)) || (rc = b_diag.alloc(8 * n)) || (rc = b_st.alloc(sizeof(sp_state)))) return rc;
    const unsigned g_rows = (unsigned)((n + SP_ROWS - 1) / SP_ROWS), g_n = (unsigned)((n + 255) / 256);
    const unsigned g_gram = (unsigned)((n + SP_GRAM_ROWS - 1) / SP_GRAM_ROWS), g_apply = (unsigned)((n + SP_APPLY_ROWS - 1) / SP_APPLY_ROWS);
    if ((rc = pcr_ensure_scratch(ctx, sizeof(double) * std::max((size_t)g_gram * SP_NG, (size_t)g_apply * SP_MAX_P)))) return rc;
    unsigned int* ticket = pcr_counter(ctx, PCR_CW_SPECTRAL_TICKET);
    sp_state* st = b_st.as<sp_state>();
    const unsigned int* indptr = g.indptr.as<const unsigned int>();
    const unsigned int* cols = g.cols.as<const unsigned int>();
    double *deg = b_deg.as<double>(), *bval = b_bval.as<double>(), *diag = b_diag.as<double>();
    PCR_HIP(ctx, hipMemsetAsync(st, 0, sizeof(sp_state), ctx->stream));
    hipLaunchKernelGGL(sp_degree_kernel, dim3(g_n), dim3(256), 0, ctx->stream, indptr, g.w.as<const double>(), n, deg, st);
    hipLaunchKernelGGL(sp_operator_kernel, dim3(g_n), dim3(256), 0, ctx->stream, indptr, cols, g.w.as<const double>(), (const double*)deg, n, normalized, (const sp_state*)st, bval,
                       diag);
    double* buf[3] = {b_buf[0].as<double>(), b_buf[1].as<double>(), b_buf[2].as<double>()};
    int cur = 0;   // the buffer that holds the block
    hipLaunchKernelGGL(sp_start_kernel, dim3(g_rows), dim3(256), 0, ctx->stream, g.rows.as<const long long>(), n, p, buf[cur]);
    PCR_HIP(ctx, hipGetLastError());
    auto spmm = [&](const double* y1, const double* y0, double* y2, double alpha, double beta, double gamma) {
        hipLaunchKernelGGL(sp_spmm_kernel, dim3(g_rows), dim3(256), 0, ctx->stream, indptr, cols, (const double*)bval, (const double*)diag, n, p, y1, y0, y2, alpha, beta, gamma);
    };
    std::vector<sp_state> h(1);
    double cut = 0.0;
    res->iters = 0;
    res->spmm = 0;
    for (int it = 0; it < params->max_iter; ++it) {
        // the scaled Chebyshev recurrence that damps [-1, cut] and is 1 at the top of the spectrum (theta = 1)
        const double e = 0.5 * (cut + 1.0), c = 0.5 * (cut - 1.0);
        double sigma = e / (1.0 - c);
        const double tau = 2.0 / sigma;
        int y0 = cur, y1 = (cur + 1) % 3, y2 = (cur + 2) % 3;
        spmm(buf[y0], nullptr, buf[y1], sigma / e, -c * (sigma / e), 0.0);
        for (int d = 2; d <= SP_DEGREE; ++d) {
            const double sn = 1.0 / (tau - sigma), alpha = 2.0 * sn / e;
            spmm(buf[y1], buf[y0], buf[y2], alpha, -c * alpha, -(sigma * sn));
            sigma = sn;
            const int t = y0; y0 = y1; y1 = y2; y2 = t;
        }
        cur = y1;
        const int other = y0;
        // columns to unit norm and Cholesky-QR, twice
        for (int rep = 0; rep < 2; ++rep) {
            hipLaunchKernelGGL(sp_gram_kernel<false>, dim3(g_gram), dim3(256), 0, ctx->stream, (const double*)buf[cur], (const double*)buf[cur], n, p, st, ctx->d_partials, ticket);
            hipLaunchKernelGGL(sp_apply_kernel<false>, dim3(g_apply), dim3(256), 0, ctx->stream, buf[cur], (double*)nullptr, n, p, m, tol2, st, ctx->d_partials, ticket);
        }
        // Rayleigh-Ritz: H = Q^T B Q, rotate Q and B Q, residuals
        spmm(buf[cur], nullptr, buf[other], 1.0, 0.0, 0.0);
        hipLaunchKernelGGL(sp_gram_kernel<true>, dim3(g_gram), dim3(256), 0, ctx->stream, (const double*)buf[cur], (const double*)buf[other], n, p, st, ctx->d_partials, ticket);
        hipLaunchKernelGGL(sp_apply_kernel<true>, dim3(g_apply), dim3(256), 0, ctx->stream, buf[cur], buf[other], n, p, m, tol2, st, ctx->d_partials, ticket);
        PCR_HIP(ctx, hipGetLastError());
        if ((rc = pcr_d2h_small(ctx, &h[0], st, SP_HEAD_BYTES))) return rc;
        res->iters = it + 1;
        res->spmm += SP_DEGREE + 1;
        if (h[0].fail) { res->bad_row = -1; return PCR_E_SINGULAR; }
        if (h[0].converged) break;
        cut = std::min(std::max(h[0].theta[p - 1], -0.9), 0.999);
    }
    const double scale = normalized ? 1.0 : __builtin_bit_cast(double, h[0].dmax_bits);
    res->converged = h[0].converged;
    res->max_degree = h[0].max_degree;
    for (int j = 0; j < m; ++j) { res->eigenvalues[j] = scale * (1.0 - h[0].theta[j]); res->residuals[j] = h[0].resid[j]; }
    res->next_eigenvalue = scale * (1.0 - h[0].theta[m]);
    hipLaunchKernelGGL(sp_embed_kernel, dim3(g_rows), dim3(256), 0, ctx->stream, (const double*)buf[cur], (const double*)deg, g.rows.as<const long long>(), n, p, m, normalized, d_E);
    hipLaunchKernelGGL(sp_colscale_kernel, dim3(1), dim3(256), 0, ctx->stream, (const double*)d_E, n, m, st->scale);
    hipLaunchKernelGGL(sp_scale_kernel, dim3((unsigned)((n * m + 255) / 256)), dim3(256), 0, ctx->stream, d_E, n, m, (const double*)st->scale);
    PCR_HIP(ctx, hipGetLastError());
    PCR_HIP(ctx, pcr_sync(ctx->stream));   // (the blocks above leave scope)
    return PCR_OK;
}

// graph -> embedding (-> K-Means when labels_out is given)
int spectral_run(pcr_ctx* ctx, const pcr_cloud* cloud, const pcr_spectral_params* params, const int64_t* seed_rows, int32_t* labels_out, double* embedding_out,
                 double* centers_out, int64_t* seed_rows_out, pcr_spectral_result* res) {
    const long long n = cloud->n;
    const int m = params->n_clusters, K = m;
    hipSetDevice(ctx->device);
    memset(res, 0, sizeof(*res));
    res->bad_row = -1;
    int rc, bad_row = -1;
    const bool dense = n <= SP_DENSE_N;
    PCR_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    sp_graph g(ctx);
    rc = sp_build_graph(ctx, cloud, params->nnk, dense, &g, &bad_row);
    res->bad_row = bad_row;
    if (rc) return rc;
    res->n_edges = g.nnz / 2;
    PCR_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    if ((rc = pcr_events_ms(ctx, &res->graph_ms))) return rc;
    PCR_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    pcr_dev_block d_E(ctx);
    if ((rc = d_E.alloc(sizeof(double) * n * m))) return rc;
    std::vector<double> h_E;
    if (dense) {
        if ((rc = dense_embed(ctx, g, m, params->normalized ? 1 : 0, h_E, res))) return rc;
        PCR_HIP(ctx, hipMemcpyAsync(d_E.p, h_E.data(), sizeof(double) * n * m, hipMemcpyHostToDevice, ctx->stream));
    } else if ((rc = device_embed(ctx, g, params, d_E.as<double>(), res))) {
        return rc;
    }
    PCR_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    if ((rc = pcr_events_ms(ctx, &res->solver_ms))) return rc;
    if (embedding_out && (rc = pcr_d2h_staged(ctx, embedding_out, d_E.p, sizeof(double) * n * m))) return rc;
    if (!labels_out) return PCR_OK;

    // ---- K-Means on the rows of the embedding
    PCR_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    pcr_stream_fit r(ctx);
    pcr_dev_block d_mind(ctx), d_labels(ctx);
    if ((rc = d_mind.alloc(8 * n)) || (rc = d_labels.alloc(4 * n))) return rc;
    std::vector<sp_km_state> h(1);
    memset(&h[0], 0, sizeof(sp_km_state));
    h[0].max_iter = params->kmeans_max_iter;
    h[0].tol = params->kmeans_tol;
    if (seed_rows) for (int j = 0; j < K; ++j) h[0].seeds[j] = seed_rows[j];
    if ((rc = pcr_stream_begin(&r, d_E.p, n, K, m, PCR_STREAM_BLOCK, PCR_CW_SPECTRAL_TICKET, &h[0], sizeof(sp_km_state), sp_row_source::NSUM))) return rc;
    sp_km_state* st = r.st.as<sp_km_state>();
    if (!seed_rows) hipLaunchKernelGGL(sp_maximin_kernel, dim3(1), dim3(256), 0, ctx->stream, d_E.as<const double>(), n, m, K, d_mind.as<double>(), st);
    hipLaunchKernelGGL(sp_km_seed_kernel, dim3(1), dim3(SP_MAX_K * SP_MAX_K), 0, ctx->stream, d_E.as<const double>(), m, K, st);
    PCR_HIP(ctx, hipGetLastError());
    if ((rc = pcr_stream_loop(&r, params->kmeans_max_iter, LLOYD_ITERS_PER_SYNC, LLOYD_HEAD_BYTES, [&](int) { return pcr_stream_launch_one(&r, sp_km_assign_kernel, m); })))
        return rc;
    if ((rc = pcr_stream_launch_one(&r, sp_km_label_kernel, m, d_labels.as<int>()))) return rc;
    PCR_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    if ((rc = pcr_d2h_small(ctx, &h[0], st, sizeof(sp_km_state)))) return rc;
    res->kmeans_iters = h[0].it;
    res->kmeans_converged = h[0].converged;
    res->n_empty = h[0].n_empty;
    res->inertia = h[0].inertia;
    if (centers_out)
        for (int k = 0; k < K; ++k)
            for (int d = 0; d < m; ++d) centers_out[k * m + d] = h[0].c[k * SP_MAX_K + d];
    if (seed_rows_out) for (int j = 0; j < K; ++j) seed_rows_out[j] = h[0].seeds[j];
    if ((rc = pcr_d2h_staged(ctx, labels_out, d_labels.p, sizeof(int32_t) * n))) return rc;
    return pcr_events_ms(ctx, &res->kmeans_ms);
}

}  // namespace

extern "C" {

void pcr_spectral_default_params(pcr_spectral_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->n_clusters = 2;
    p->nnk = 7;
    p->normalized = 1;
    p->max_iter = 200;
    p->kmeans_max_iter = 300;
    p->tol = 1e-8;
    p->kmeans_tol = 1e-4;
}

int pcr_sym_eig_jacobi(int n, const double* A, double* eigvals_out, double* eigvecs_out) try {
    if (n < 1 || n > SP_DENSE_N || !A || !eigvals_out || !eigvecs_out) return PCR_E_INVALID;
    std::vector<double> a((size_t)n * n), v((size_t)n * n);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) a[(size_t)i * n + j] = 0.5 * (A[(size_t)i * n + j] + A[(size_t)j * n + i]);
    pcr_jacobi_eig(n, a.data(), v.data(), 0, 1, [] {});
    std::vector<int> order(n);
    pcr_order_desc(n, a.data(), order.data());
    for (int j = 0; j < n; ++j) {   // ascending
        const int o = order[n - 1 - j];
        eigvals_out[j] = a[(size_t)o * n + o];
        for (int i = 0; i < n; ++i) eigvecs_out[(size_t)i * n + j] = v[(size_t)i * n + o];
    }
    return PCR_OK;
} PCR_CATCH((pcr_ctx*)nullptr)

int pcr_knn_graph(pcr_ctx* ctx, const pcr_cloud* cloud, int nnk, int64_t* indptr_out, int32_t* indices_out, double* weights_out, int32_t* bad_row_out) try {
    if (!ctx || !cloud || !indptr_out || (indices_out && !weights_out) || nnk < 1 || nnk > PCR_SPECTRAL_MAX_NNK) return PCR_E_INVALID;
    int rc;
    if ((rc = cloud_ok(cloud, nnk, 1, nullptr))) return rc;
    hipSetDevice(ctx->device);
    const int64_t n = cloud->n;
    sp_graph g(ctx);
    int bad_row = -1;
    rc = sp_build_graph(ctx, cloud, nnk, true, &g, &bad_row);
    if (bad_row_out) *bad_row_out = bad_row;
    if (rc) return rc;
    std::vector<unsigned int> indptr((size_t)n + 1);
    PCR_HIP(ctx, hipMemcpyAsync(indptr.data(), g.indptr.p, 4 * (size_t)(n + 1), hipMemcpyDeviceToHost, ctx->stream));
    PCR_HIP(ctx, pcr_sync(ctx->stream));
    for (int64_t i = 0; i <= n; ++i) indptr_out[i] = indptr[(size_t)i];
    if (!indices_out) return PCR_OK;
    if ((rc = pcr_d2h_staged(ctx, indices_out, g.cols.p, 4 * (size_t)g.nnz)) || (rc = pcr_d2h_staged(ctx, weights_out, g.w.p, 8 * (size_t)g.nnz))) return rc;
    return PCR_OK;
} PCR_CATCH(ctx)

int pcr_spectral_embed(pcr_ctx* ctx, const pcr_cloud* cloud, const pcr_spectral_params* params, double* embedding_out, pcr_spectral_result* result) try {
    if (!ctx || !cloud || !params || !embedding_out || !result || !params_ok(params)) return PCR_E_INVALID;
    int rc;
    if ((rc = cloud_ok(cloud, params->nnk, params->n_clusters, nullptr))) return rc;
    return spectral_run(ctx, cloud, params, nullptr, nullptr, embedding_out, nullptr, nullptr, result);
} PCR_CATCH(ctx)

int pcr_spectral_fit(pcr_ctx* ctx, const pcr_cloud* cloud, const pcr_spectral_params* params, const int64_t* seed_rows, int32_t* labels_out, double* embedding_out,
                     double* centers_out, int64_t* seed_rows_out, pcr_spectral_result* result) try {
    if (!ctx || !cloud || !params || !labels_out || !result || !params_ok(params)) return PCR_E_INVALID;
    int rc;
    if ((rc = cloud_ok(cloud, params->nnk, params->n_clusters, seed_rows))) return rc;
    return spectral_run(ctx, cloud, params, seed_rows, labels_out, embedding_out, centers_out, seed_rows_out, result);
} PCR_CATCH(ctx)

}  // extern "C"
