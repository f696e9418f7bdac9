// PCL-rule FPFH33 at keypoint POSITIONS -- featureFPFH33 / featureFPFH33WithNormal of PCLKeypoints/src/keypoints.cpp, by the rules
// stated in include/pcr.h (PCL itself is not part of the build: parity with its binary32 output is unpinned).  The keypoints are
// coordinates searched against the cloud as search surface, the neighbourhood is the radius ball alone and has no cap, the weighted
// sum is normalised and nothing is added to it.
// The surface is indexed by the grid with cell = radius over a caller-row-order copy (ball_grid), so a ball lies in the 3x3x3 block of
// its centre's cell and a cell's records stand in caller-row order.  A ball is WALKED, never stored: one wave per centre, by the wave
// walk of pcr_ball_visit.h (the 27 runs one after the other, 64 records a trip).  Four stages on the stream, nothing read back
// between them:
//   mark      wave per keypoint: need[position] = 1 for the records of its ball (plain stores of one constant), the ball's size
//   compact   rocprim::select over the positions: the marked records in ascending position, their number M on the device
//   SPFH      wave per marked record: the in-ball positions of a trip are compacted into LDS (ballot + prefix) and the pair features
//             are taken 64 at a time, every lane busy; integer LDS counts -> spfh[k] = count * (100 / (K - 1)); need[] becomes slot[]
//   FPFH      wave per keypoint: the in-ball (slot, d^2) with d^2 != 0 are staged in LDS in walk order; lane = bin adds spfh / d^2 over
//             the staged entries in that order, then the three block sums and the scaling
// A record is named by its POSITION in the grid's order, not by its row: the stages hand positions to each other and need no
// row -> position table; only the normals (the caller's, by row) are fetched by row.  Walk order = block cell 0..26, then stored
// order: a function of the surface in caller-row order and of the radius, not of the keypoints -- the FPFH sums are repeatable to the
// bit and the same for a keypoint whichever others are asked for.  The SPFH counts are integers and combine in any order.
#include <cmath>
#include <cstring>
#include <string>
#include "pcr_ball_visit.h"
#include "pcr_pair_features.h"
#include "pcr_sort.h"

constexpr int SP_STAGE = 128;   // staged in-ball positions of the SPFH pass: < 64 left over + <= 64 of a trip
constexpr int FP_STAGE = 256;   // staged (slot, d^2) of the FPFH pass, consumed when another trip might not fit

__global__ void __launch_bounds__(64) pcl_mark_kernel(pcr_grid_view gv, const double* __restrict__ kp /* (m,3) */, double r2, unsigned int* __restrict__ need /* by position, zeroed */,
                                                      int* __restrict__ counts /* (m) */) {
    const int lane = threadIdx.x;
    const long long i = blockIdx.x;
    const double x = kp[3 * i], y = kp[3 * i + 1], z = kp[3 * i + 2];
    unsigned int s, e;
    wave_block_runs(gv, x, y, z, lane, &s, &e);
    int c = 0;
    auto f = [&](unsigned int j, bool valid) {
        if (valid && dist2(x, y, z, gv.pts[j]) <= r2) { need[j] = 1u; ++c; }
    };
    wave_visit_runs(s, e, lane, f);
    c = wave_sum_all(c);
    if (lane == 0) counts[i] = c;
}

__global__ void __launch_bounds__(64) pcl_spfh_kernel(pcr_grid_view gv, double r2, const double* __restrict__ normals /* by row */, const unsigned int* __restrict__ marked,
                                                      const unsigned int* __restrict__ n_marked, unsigned int* __restrict__ slot /* by position: was `need` */,
                                                      double* __restrict__ spfh /* (>= M,33) */) {
    __shared__ unsigned int s_pos[SP_STAGE];
    __shared__ int hist[33];
    const int lane = threadIdx.x;
    const unsigned int k = blockIdx.x;
    if (k >= *n_marked) return;
    const unsigned int pos = marked[k];
    const pcr_pt p = gv.pts[pos];
    if (lane == 0) slot[pos] = k;
    if (lane < 33) hist[lane] = 0;
    const double p1[3] = {p.x, p.y, p.z};
    const double n1[3] = {normals[3 * p.id], normals[3 * p.id + 1], normals[3 * p.id + 2]};
    const bool ok1 = finite3(n1[0], n1[1], n1[2]);
    // a pair is binned, or skipped: the row itself (by row number), a non-finite normal on either side, zero length, zero cross product
    auto pair = [&](unsigned int j) {
        const pcr_pt b = gv.pts[j];
        if (b.id == p.id || !ok1) return;
        const double n2[3] = {normals[3 * b.id], normals[3 * b.id + 1], normals[3 * b.id + 2]};
        if (!finite3(n2[0], n2[1], n2[2])) return;
        const double p2[3] = {b.x, b.y, b.z};
        double f[3];
        if (!pair_features(p1, n1, p2, n2, f)) return;
        int bins[3];
        pair_bins(f, bins);
        atomicAdd(&hist[bins[0]], 1);
        atomicAdd(&hist[bins[1]], 1);
        atomicAdd(&hist[bins[2]], 1);
    };
    unsigned int s, e;
    wave_block_runs(gv, p.x, p.y, p.z, lane, &s, &e);
    int staged = 0, K = 0;   // (the same in every lane)
    __syncthreads();
    auto trip = [&](unsigned int j, bool valid) {
        const bool in = valid && dist2(p.x, p.y, p.z, gv.pts[j]) <= r2;
        int add;
        const int at = staged + wave_compact_slot(in, lane, &add);
        if (in) s_pos[at] = j;
        staged += add;
        K += add;
        if (staged >= 64) {
            __syncthreads();
            pair(s_pos[staged - 64 + lane]);
            staged -= 64;
            __syncthreads();
        }
    };
    wave_visit_runs(s, e, lane, trip);
    __syncthreads();
    if (lane < staged) pair(s_pos[lane]);
    __syncthreads();
    if (lane < 33) spfh[33 * (size_t)k + lane] = K > 1 ? (double)hist[lane] * (100.0 / (double)(K - 1)) : 0.0;
}

__global__ void __launch_bounds__(64) pcl_fpfh_kernel(pcr_grid_view gv, const double* __restrict__ kp /* (m,3) */, double r2, const unsigned int* __restrict__ slot /* by position */,
                                                      const double* __restrict__ spfh, const int* __restrict__ counts /* (m) */, double* __restrict__ out /* (m,33) */) {
    __shared__ unsigned int s_slot[FP_STAGE];
    __shared__ double s_d2[FP_STAGE];
    __shared__ double s_acc[33];
    const int lane = threadIdx.x;
    const long long i = blockIdx.x;
    if (counts[i] == 0) {   // an empty ball, or a keypoint that is not finite
        if (lane < 33) out[33 * i + lane] = NAN;
        return;
    }
    const double x = kp[3 * i], y = kp[3 * i + 1], z = kp[3 * i + 2];
    unsigned int s, e;
    wave_block_runs(gv, x, y, z, lane, &s, &e);
    int staged = 0;   // (the same in every lane)
    double acc = 0.0;
    // lane = bin: the staged terms in their order, the SPFH rows of eight entries requested together
    auto consume = [&]() {
        if (lane >= 33) return;
        int t = 0;
        for (; t + 8 <= staged; t += 8) {
            double v[8], d[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) { d[u] = s_d2[t + u]; v[u] = spfh[33 * (size_t)s_slot[t + u] + lane]; }
#pragma unroll
            for (int u = 0; u < 8; ++u) acc += v[u] / d[u];
        }
        for (; t < staged; ++t) acc += spfh[33 * (size_t)s_slot[t] + lane] / s_d2[t];
    };
    auto trip = [&](unsigned int j, bool valid) {
        double d2 = 0.0;
        bool in = false;
        if (valid) {
            d2 = dist2(x, y, z, gv.pts[j]);
            in = d2 <= r2 && d2 != 0.0;   // (a row at distance 0 is in the ball and adds nothing)
        }
        int add;
        const int at = staged + wave_compact_slot(in, lane, &add);
        if (in) {
            s_slot[at] = slot[j];
            s_d2[at] = d2;
        }
        staged += add;
        if (staged + 64 > FP_STAGE) {
            __syncthreads();
            consume();
            staged = 0;
            __syncthreads();
        }
    };
    wave_visit_runs(s, e, lane, trip);
    __syncthreads();
    consume();
    if (lane < 33) s_acc[lane] = acc;
    __syncthreads();
    if (lane < 33) {
        const int g = lane / 11;
        double sum = 0.0;
#pragma unroll
        for (int b = 0; b < 11; ++b) sum += s_acc[11 * g + b];
        out[33 * i + lane] = acc * (sum != 0.0 ? 100.0 / sum : 0.0);
    }
}

extern "C" int pcr_fpfh_pcl(pcr_ctx* ctx, const pcr_cloud* surface, const double* normals, const double* keypoints, int64_t m, double radius, double* features_out,
                            int32_t* counts_out, int64_t* n_spfh_out) try {
    if (!ctx || !surface || !normals || m < 0 || !(radius > 0) || !std::isfinite(radius)) return PCR_E_INVALID;
    if (m > 0 && (!keypoints || !features_out)) return PCR_E_INVALID;
    if (m > 0x7fffffffLL) return PCR_E_INVALID;   // (one block per keypoint)
    if (surface->n <= 0) return PCR_E_EMPTY;
    if (m == 0) { if (n_spfh_out) *n_spfh_out = 0; return PCR_OK; }
    hipSetDevice(ctx->device);
    const int64_t n = surface->n;
    pcr_index_guard idx(ctx);
    int rc = ball_grid(ctx, surface, radius, "pcr_fpfh_pcl", idx);
    if (rc) return rc;
    // The (M,33) block is sized by n: M is known on the device only, and reading it back in front of the SPFH launch would put a
    // second host wait into the call (264 n bytes from the arena instead of 264 M; blocks k >= M of the SPFH launch leave at once).
    pcr_dev_block b_nrm(ctx), b_kp(ctx), b_need(ctx), b_marked(ctx), b_m(ctx), b_spfh(ctx), b_counts(ctx), b_out(ctx), b_tmp(ctx);
    if ((rc = b_nrm.alloc(sizeof(double) * 3 * n)) || (rc = b_kp.alloc(sizeof(double) * 3 * m)) || (rc = b_need.alloc(sizeof(unsigned int) * n)) ||
        (rc = b_marked.alloc(sizeof(unsigned int) * n)) || (rc = b_m.alloc(16)) || (rc = b_counts.alloc(sizeof(int) * m)) || (rc = b_out.alloc(sizeof(double) * 33 * m)) ||
        (rc = b_spfh.alloc(sizeof(double) * 33 * n)))
        return rc;
    const double r2 = radius * radius;
    PCR_HIP(ctx, hipMemcpyAsync(b_nrm.p, normals, sizeof(double) * 3 * n, hipMemcpyHostToDevice, ctx->stream));
    PCR_HIP(ctx, hipMemcpyAsync(b_kp.p, keypoints, sizeof(double) * 3 * m, hipMemcpyHostToDevice, ctx->stream));
    PCR_HIP(ctx, hipMemsetAsync(b_need.p, 0, sizeof(unsigned int) * n, ctx->stream));
    pcr_prof_mark(ctx, 0);
    hipLaunchKernelGGL(pcl_mark_kernel, dim3((unsigned)m), dim3(64), 0, ctx->stream, idx->view, (const double*)b_kp.p, r2, b_need.as<unsigned int>(), b_counts.as<int>());
    pcr_prof_mark(ctx, 1);
    if ((rc = pcr_select_positions(ctx, b_need.as<unsigned int>(), (size_t)n, b_marked.as<unsigned int>(), b_m.as<unsigned int>(), b_tmp))) return rc;
    pcr_prof_mark(ctx, 2);
    hipLaunchKernelGGL(pcl_spfh_kernel, dim3((unsigned)n), dim3(64), 0, ctx->stream, idx->view, r2, (const double*)b_nrm.p, (const unsigned int*)b_marked.p,
                       (const unsigned int*)b_m.p, b_need.as<unsigned int>(), b_spfh.as<double>());
    pcr_prof_mark(ctx, 3);
    hipLaunchKernelGGL(pcl_fpfh_kernel, dim3((unsigned)m), dim3(64), 0, ctx->stream, idx->view, (const double*)b_kp.p, r2, (const unsigned int*)b_need.p,
                       (const double*)b_spfh.p, (const int*)b_counts.p, b_out.as<double>());
    pcr_prof_mark(ctx, 4);
    PCR_HIP(ctx, hipGetLastError());
    // (the downloads are enqueued behind the kernels; the read of M is the call's one wait)
    PCR_HIP(ctx, hipMemcpyAsync(features_out, b_out.p, sizeof(double) * 33 * m, hipMemcpyDeviceToHost, ctx->stream));
    if (counts_out) PCR_HIP(ctx, hipMemcpyAsync(counts_out, b_counts.p, sizeof(int) * m, hipMemcpyDeviceToHost, ctx->stream));
    unsigned int n_marked = 0;
    if ((rc = pcr_d2h_small(ctx, &n_marked, b_m.p, sizeof(unsigned int)))) return rc;   // (synchronises)
    pcr_prof_finish(ctx);
    if (n_spfh_out) *n_spfh_out = (int64_t)n_marked;
    return PCR_OK;
} PCR_CATCH(ctx)
