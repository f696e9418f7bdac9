// Point-to-plane ICP refinement: refine_registration, Registration/main.py:87-95 = Open3D registration_icp with
// TransformationEstimationPointToPlane (semantics and deviations: include/pcr.h).
//
// Per pass the existing exact 1-NN search runs unchanged (pcr_grid_nn1 / pcr_brute_nn1: target row per source row, -1 behind the
// gate, left on the device), then ONE launch of point2plane_accumulate_kernel: every source record is transformed by the composed T
// in registers (the cloud is never written), its matched target point and normal are fetched by the same position, and 29 binary64
// sums are accumulated -- the 21 upper entries of A = sum J J^T, the 6 of b = sum J r, K and sum d^2.  No floating-point atomics:
// per-thread sums in grid-stride order, wave totals on the DPP network, a fixed tree over the block's four waves, block slabs in
// ctx->d_partials, and the block that takes the last ticket adds the slabs in block order -- two calls on the same inputs give the
// same bits.  One lane of that block then finishes the pass: evaluation (fitness, inlier_rmse), the stop rule, the 6x6 LDL^T solve,
// U, T <- U T, and the loop state the next pass reads.  The host reads the head of that state (168 bytes) once per iteration, because
// the search takes its transform as a launch argument; no per-point data leaves the device.
#include <cmath>
#include <cstring>
#include "pcr_internal.h"
#include "pcr_linalg.h"
#include "pcr_icp_step.h"
#include "pcr_stream_fit.h"   // pcr_events_ms
#include "pcr_wave.h"
#include "pcr_grid_dev.h"     // xform_apply

namespace {

constexpr int P2P_NSUM = 29;         // A upper triangle (21), b (6), K, sum d^2

// Loop state on the device.  The head (everything before the logs) is what the host reads every iteration.
struct __attribute__((aligned(16))) p2p_state {
    double T[16];          // composed transform the NEXT pass applies
    double fitness, rmse;  // last evaluation
    long long n_corr;
    int it;                // updates performed
    int stop;              // no further pass may run
    int status;
    int passes;            // evaluations performed
    double fitness_log[PCR_ICP_MAX_LOG + 1], rmse_log[PCR_ICP_MAX_LOG + 1];
};
constexpr size_t P2P_HEAD_BYTES = offsetof(p2p_state, fitness_log);
static_assert(P2P_HEAD_BYTES <= 512, "the per-iteration read-back stays below 512 bytes");
static_assert(sizeof(p2p_state) <= PCR_SMALL_D2H_BYTES && sizeof(p2p_state) % 8 == 0, "state read back through pcr_d2h_small");

struct p2p_loop_args {
    int max_iter;
    double rel_fitness, rel_rmse;
};
struct p2p_T { double v[16]; };

// End of a pass, one lane: `s` = the 29 sums of the evaluation of st->T.
__device__ void p2p_finish_pass(p2p_state* __restrict__ st, const double* s, long long nq, const p2p_loop_args la) {
    const long long K = (long long)llrint(s[27]);
    const double fitness = K > 0 ? (double)K / (double)nq : 0.0;
    const double rmse = K > 0 ? sqrt(s[28] / (double)K) : 0.0;
    const int pass = st->passes;   // 0: the evaluation of T0, i: the evaluation behind update i
    const bool converged = pass > 0 && fabs(st->fitness - fitness) < la.rel_fitness && fabs(st->rmse - rmse) < la.rel_rmse;
    st->fitness = fitness;
    st->rmse = rmse;
    st->n_corr = K;
    st->fitness_log[pass] = fitness;
    st->rmse_log[pass] = rmse;
    st->passes = pass + 1;
    if (converged || pass >= la.max_iter) { st->stop = 1; return; }
    double x[6], U[16];
    if (K < 6 || !pcr::point2plane_solve(s, s + 21, x, U)) {   // stated deviation: identity update, soft status, stop
        st->status = PCR_E_TOO_FEW_ASSOC;
        st->stop = 1;
        return;
    }
    double T[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) T[i] = st->T[i];
    pcr::T_mul4(U, T, T);
#pragma unroll
    for (int i = 0; i < 16; ++i) st->T[i] = T[i];
    st->it = pass + 1;
}

// q: source records (any order; id = caller row).  nn_idx: matched target ROW per source row (-1: no correspondence).  tgt / nrm:
// target records and normals by position; row_pos: position of a target row (null: position = row).
// st != null: the loop (transform = st->T, the last block finishes the pass); st == null: one pass with `T_arg`, sums to `out`.
__global__ void __launch_bounds__(256)
point2plane_accumulate_kernel(const pcr_pt* __restrict__ q, long long nq, const int* __restrict__ nn_idx, const pcr_pt* __restrict__ tgt,
                              const double* __restrict__ nrm, const int* __restrict__ row_pos, p2p_T T_arg, double* __restrict__ partials,
                              unsigned int* __restrict__ ticket, double* __restrict__ out, p2p_state* __restrict__ st, p2p_loop_args la) {
    __shared__ double s_part[4][P2P_NSUM], s_red[8][P2P_NSUM], s_tot[P2P_NSUM];
    if (st && st->stop) return;
    pcr_xform x;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) x.r[3 * i + j] = st ? st->T[4 * i + j] : T_arg.v[4 * i + j];
        x.t[i] = st ? st->T[4 * i + 3] : T_arg.v[4 * i + 3];
    }
    double m[P2P_NSUM];
#pragma unroll
    for (int k = 0; k < P2P_NSUM; ++k) m[k] = 0.0;
    // batches of 4 records per thread: the 4 source records, the 4 matches, the 4 positions and then the 4 target points and
    // normals are each loaded together (dependent round trips per batch, not per record)
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long q0 = (long long)blockIdx.x * blockDim.x + threadIdx.x; q0 < nq; q0 += 4 * stride) {
        pcr_pt p[4];
        int pos[4];
        double bx[4], by[4], bz[4], nx[4], ny[4], nz[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long qi = q0 + u * stride;
            pos[u] = -1;
            if (qi < nq) p[u] = q[qi];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (q0 + u * stride < nq) pos[u] = nn_idx[p[u].id];
        if (row_pos) {
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (pos[u] >= 0) pos[u] = row_pos[pos[u]];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (pos[u] < 0) continue;
            const pcr_pt b = tgt[pos[u]];
            bx[u] = b.x; by[u] = b.y; bz[u] = b.z;
            nx[u] = nrm[3ll * pos[u]]; ny[u] = nrm[3ll * pos[u] + 1]; nz[u] = nrm[3ll * pos[u] + 2];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (pos[u] < 0) continue;
            double sx, sy, sz;
            xform_apply(x, p[u], &sx, &sy, &sz);
            const double dx = sx - bx[u], dy = sy - by[u], dz = sz - bz[u];
            const double r = (dx * nx[u] + dy * ny[u]) + dz * nz[u];
            const double J[6] = {sy * nz[u] - sz * ny[u], sz * nx[u] - sx * nz[u], sx * ny[u] - sy * nx[u], nx[u], ny[u], nz[u]};
            int k = 0;
#pragma unroll
            for (int i = 0; i < 6; ++i)
#pragma unroll
                for (int j = i; j < 6; ++j) m[k++] += J[i] * J[j];
#pragma unroll
            for (int i = 0; i < 6; ++i) m[21 + i] += J[i] * r;
            m[27] += 1.0;
            m[28] += (dx * dx + dy * dy) + dz * dz;
        }
    }
#pragma unroll
    for (int k = 0; k < P2P_NSUM; ++k) m[k] = wave_total_f64(m[k]);   // total in lane 63, fixed order
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 63) {
#pragma unroll
        for (int k = 0; k < P2P_NSUM; ++k) s_part[wave][k] = m[k];
    }
    // one slab per block; the block that arrives last adds the slabs in a fixed order
    if (!block_slab_sums<P2P_NSUM>(s_part, P2P_NSUM, partials, ticket, s_red, s_tot, [](double a, double b, int) { return a + b; })) return;
    if (out && threadIdx.x < P2P_NSUM) out[threadIdx.x] = s_tot[threadIdx.x];
    if (st && threadIdx.x == 0) p2p_finish_pass(st, s_tot, nq, la);
}

// loop state before the first pass: zero, T = T0
__global__ void __launch_bounds__(256) point2plane_init_kernel(p2p_state* __restrict__ st, p2p_T T0) {
    unsigned long long* w = reinterpret_cast<unsigned long long*>(st);
    for (unsigned int i = threadIdx.x; i < sizeof(p2p_state) / 8; i += blockDim.x) w[i] = 0ull;
    __syncthreads();
    if (threadIdx.x < 16) st->T[threadIdx.x] = T0.v[threadIdx.x];
}

// normals by target row -> by position of `rec` (id = row), and the position of every row
__global__ void __launch_bounds__(256) point2plane_permute_normals_kernel(const pcr_pt* __restrict__ rec, long long n, const double* __restrict__ by_row,
                                                                           double* __restrict__ by_pos, int* __restrict__ row_pos) {
    const long long pos = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (pos >= n) return;
    const long long row = rec[pos].id;
    by_pos[3 * pos] = by_row[3 * row];
    by_pos[3 * pos + 1] = by_row[3 * row + 1];
    by_pos[3 * pos + 2] = by_row[3 * row + 2];
    row_pos[row] = (int)pos;
}

// scratch of a call: the search's results by source row
struct p2p_scratch {
    pcr_dev_block nn_idx, nn_d2;
    int grid = 1;
    explicit p2p_scratch(pcr_ctx* ctx) : nn_idx(ctx), nn_d2(ctx) {}
};

int p2p_prepare(pcr_ctx* ctx, int64_t nq, p2p_scratch* sc) {
    int rc;
    if ((rc = sc->nn_idx.alloc(sizeof(int32_t) * nq)) || (rc = sc->nn_d2.alloc(sizeof(double) * nq))) return rc;
    sc->grid = (int)((nq + 1023) / 1024);  // four records per thread, at most one block per CU (<= 256 slabs)
    const int cap = ctx->cu_count < 256 ? ctx->cu_count : 256;
    if (sc->grid > cap) sc->grid = cap;
    return pcr_ensure_scratch(ctx, sizeof(double) * P2P_NSUM * (size_t)sc->grid);
}

// the unchanged search, then the accumulate launch.  T: the transform the search applies (the loop's kernel reads the same from st)
int p2p_pass(pcr_ctx* ctx, pcr_cloud* source, const pcr_index* index, const double T[16], double max_d2, const p2p_scratch* sc, double* d_out,
             p2p_state* d_st, const p2p_loop_args& la) {
    pcr_xform x;
    pcr_xform_from_T(T, &x);
    int rc;
    if (index->kind == PCR_INDEX_GRID) rc = pcr_grid_nn1(ctx, index, source, &x, max_d2, sc->nn_idx.as<int32_t>(), sc->nn_d2.as<double>());
    else rc = pcr_brute_nn1(ctx, index, source->d, source->n, &x, max_d2, sc->nn_idx.as<int32_t>(), sc->nn_d2.as<double>());
    if (rc) return rc;
    p2p_T Ta;
    memcpy(Ta.v, T, sizeof(Ta.v));
    const bool grid = index->kind == PCR_INDEX_GRID;
    hipLaunchKernelGGL(point2plane_accumulate_kernel, dim3(sc->grid), dim3(256), 0, ctx->stream, (const pcr_pt*)source->d, (long long)source->n,
                       (const int*)sc->nn_idx.p, (const pcr_pt*)(grid ? index->sorted : index->plain), (const double*)index->normals,
                       (const int*)(grid ? index->row_pos : nullptr), Ta, ctx->d_partials, pcr_counter(ctx, PCR_CW_P2P_TICKET), d_out, d_st, la);
    PCR_HIP(ctx, hipGetLastError());
    return PCR_OK;
}

double gate_d2(double max_dist) { return (max_dist > 0 && std::isfinite(max_dist)) ? max_dist * max_dist : 0.0; }

}  // namespace

void pcr_point2plane_free(pcr_ctx* ctx, pcr_index* idx) {
    if (idx->normals) pcr_dev_free(ctx, idx->normals);
    if (idx->row_pos) pcr_dev_free(ctx, idx->row_pos);
    idx->normals = nullptr;
    idx->row_pos = nullptr;
}

extern "C" {

int pcr_index_has_normals(const pcr_index* index) { return (index && index->normals) ? 1 : 0; }

int pcr_index_set_normals(pcr_ctx* ctx, pcr_index* index, const double* normals) {
    if (!ctx || !index || !normals) return PCR_E_INVALID;
    const int64_t n = index->n;
    for (int64_t i = 0; i < 3 * n; ++i)
        if (!std::isfinite(normals[i])) return PCR_E_INVALID;
    hipSetDevice(ctx->device);
    int rc;
    const bool grid = index->kind == PCR_INDEX_GRID;
    pcr_dev_block by_row(ctx);   // (taken before the index's own blocks: a refusal here leaves the index as it was)
    if (grid && (rc = by_row.alloc(sizeof(double) * 3 * n))) return rc;
    if (!index->normals && (rc = pcr_dev_alloc(ctx, sizeof(double) * 3 * n, (void**)&index->normals))) return rc;
    if (grid && !index->row_pos && (rc = pcr_dev_alloc(ctx, sizeof(int32_t) * n, (void**)&index->row_pos))) {
        pcr_point2plane_free(ctx, index);
        return rc;
    }
    if (!grid) {   // `plain` is in row order already
        PCR_HIP(ctx, hipMemcpyAsync(index->normals, normals, sizeof(double) * 3 * n, hipMemcpyHostToDevice, ctx->stream));
        PCR_HIP(ctx, pcr_sync(ctx->stream));
        return PCR_OK;
    }
    PCR_HIP(ctx, hipMemcpyAsync(by_row.p, normals, sizeof(double) * 3 * n, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(point2plane_permute_normals_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, (const pcr_pt*)index->sorted,
                       (long long)n, (const double*)by_row.p, index->normals, index->row_pos);
    PCR_HIP(ctx, hipGetLastError());
    PCR_HIP(ctx, pcr_sync(ctx->stream));   // the caller's array has been read
    return PCR_OK;
}

void pcr_icp_plane_default_params(pcr_icp_plane_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->max_iter = 30;        // Open3D ICPConvergenceCriteria defaults (Registration/main.py:92-94 passes none)
    p->rel_fitness = 1e-6;
    p->rel_rmse = 1e-6;
    p->max_dist = 0.0;
}

int pcr_point2plane_moments(pcr_ctx* ctx, const pcr_cloud* source, const pcr_index* index, const double* T, double max_dist, double out[29]) try {
    if (!ctx || !source || !index || !out || !index->normals) return PCR_E_INVALID;
    if (source->n <= 0) return PCR_E_EMPTY;
    hipSetDevice(ctx->device);
    const double I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    p2p_scratch sc(ctx);
    pcr_dev_block d_out(ctx);
    int rc;
    if ((rc = p2p_prepare(ctx, source->n, &sc)) || (rc = d_out.alloc(sizeof(double) * P2P_NSUM))) return rc;
    if ((rc = p2p_pass(ctx, const_cast<pcr_cloud*>(source), index, T ? T : I, gate_d2(max_dist), &sc, d_out.as<double>(), nullptr, p2p_loop_args{})))
        return rc;
    return pcr_d2h_small(ctx, out, d_out.p, sizeof(double) * P2P_NSUM);
} PCR_CATCH(ctx)

int pcr_icp_point2plane(pcr_ctx* ctx, const pcr_cloud* source, const pcr_index* index, const pcr_icp_plane_params* params, const double T0[16],
                        pcr_icp_plane_result* res) try {
    if (!ctx || !source || !index || !params || !T0 || !res) return PCR_E_INVALID;
    if (!index->normals || params->max_iter < 0) return PCR_E_INVALID;
    if (params->max_iter > PCR_ICP_MAX_LOG) return PCR_E_TOO_MANY_ITERS;
    if (source->n <= 0) return PCR_E_EMPTY;
    hipSetDevice(ctx->device);
    memset(res, 0, sizeof(*res));
    pcr_cloud* src = const_cast<pcr_cloud*>(source);   // the search may lay the records out along the query curve: rows and values stay
    p2p_scratch sc(ctx);
    pcr_dev_block d_st(ctx);
    int rc;
    if ((rc = p2p_prepare(ctx, source->n, &sc)) || (rc = d_st.alloc(sizeof(p2p_state)))) return rc;
    if (index->kind == PCR_INDEX_GRID && (rc = pcr_cloud_morton_sort(ctx, src, index->cell))) return rc;   // outside the timed loop
    const p2p_loop_args la{params->max_iter, params->rel_fitness, params->rel_rmse};
    const double max_d2 = gate_d2(params->max_dist);
    PCR_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    p2p_T T;
    memcpy(T.v, T0, sizeof(T.v));
    hipLaunchKernelGGL(point2plane_init_kernel, dim3(1), dim3(256), 0, ctx->stream, d_st.as<p2p_state>(), T);
    PCR_HIP(ctx, hipGetLastError());
    p2p_state head;   // only the head is read inside the loop
    for (int pass = 0; pass <= params->max_iter; ++pass) {
        if ((rc = p2p_pass(ctx, src, index, T.v, max_d2, &sc, nullptr, d_st.as<p2p_state>(), la))) return rc;
        // one synchronisation per iteration: the next search takes T as a launch argument
        if ((rc = pcr_d2h_small(ctx, &head, d_st.p, P2P_HEAD_BYTES))) return rc;
        memcpy(T.v, head.T, sizeof(T.v));
        if (head.stop) break;
    }
    PCR_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    p2p_state* full = new p2p_state;
    rc = pcr_d2h_small(ctx, full, d_st.p, sizeof(p2p_state));
    if (rc == PCR_OK) {
        memcpy(res->T, full->T, sizeof(res->T));
        res->fitness = full->fitness;
        res->inlier_rmse = full->rmse;
        res->n_corr = full->n_corr;
        res->iters = full->it;
        res->status = full->status;
        res->nn_launches = full->passes;
        for (int i = 0; i < full->passes && i <= PCR_ICP_MAX_LOG; ++i) { res->fitness_log[i] = full->fitness_log[i]; res->rmse_log[i] = full->rmse_log[i]; }
    }
    delete full;
    if (rc) return rc;
    if ((rc = pcr_events_ms(ctx, &res->device_ms))) return rc;
    return res->status;
} PCR_CATCH(ctx)

int pcr_point2plane_solve(const double A_upper[21], const double b[6], double x[6], double U[16]) {
    if (!A_upper || !b || !x || !U) return PCR_E_INVALID;
    return pcr::point2plane_solve(A_upper, b, x, U) ? PCR_OK : PCR_E_TOO_FEW_ASSOC;
}

}  // extern "C"
