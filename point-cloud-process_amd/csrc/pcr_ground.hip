// Ground segmentation: the RANSAC plane removal of Cluster_dbscan/clustering.py:36-95 on a device-resident cloud.
//
// The caller supplies the sampled rows (clustering.py:57 draws them from np.random; the library has no generator for this step), so
// every hypothesis is known up front and the reference's sequential loop becomes: score ALL hypotheses in one streaming pass, then
// apply its running-best / early-break rule (clustering.py:75-81) to the counts.  Launches, all on the context's stream with no host
// round trip before the counts are final and the winner is masked:
//   pcr_cloud_gather_rows (Morton-reordered clouds only) the sampled points by caller row: position != row there, so every record
//                         looks its id up in the sorted list of distinct sampled rows (pcr_core.hip);
//   ground_setup_kernel   p0 and the unit normal of every hypothesis (pcr_ground_plane_from), counters zeroed;
//   ground_score_kernel   one launch per chunk of GR_CHUNK hypotheses (the default 35 are one): 32 B per point read once, the chunk's
//                         planes broadcast from LDS, per wave one integer count per hypothesis (popcount of the wave's ballots, scalar
//                         arithmetic), one integer atomic add per hypothesis per block; the block that takes the last ticket of the
//                         last chunk runs pcr_ground_select's rule on the device;
//   ground_mask_kernel    the winner evaluated once more with the SAME distance function, flag by caller row;
//   ground_scan_kernel / ground_offsets_kernel / ground_scatter_kernel   stable compaction of the outlier rows in ascending row order.
// Counts are integers: no floating-point atomics, no dependence on arrival order.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>
#include "pcr_internal.h"
#include "pcr_wave.h"

namespace {

constexpr int GR_CHUNK = 256;       // hypotheses per scoring launch: their planes and counters sit in LDS (13 KiB)
constexpr int GR_PTS = 4;           // points per lane of the scoring pass, in registers while the chunk's planes go by
constexpr int GR_BLOCK = PCR_STREAM_BLOCK;
constexpr int GR_TILE = 1024;       // rows per block of the compaction scan (4 per thread)

struct gr_plane { double p[3], n[3]; };   // p0 and unit normal (NaN for a degenerate triple, clustering.py:61-62)

struct gr_state {
    int best_hyp, evaluated, status, pad;
    long long n_inliers, n_outliers, scan_total;
    gr_plane plane;
};

// clustering.py:59-62: k1 = p0 - p1, k2 = p0 - p2, n = cross(k1, k2) / ||.||, in the operation order fixed in DESIGN (no contraction).
// A zero cross product gives 0/0 = NaN in every component, like the reference.
__host__ __device__ inline gr_plane pcr_ground_plane_from(const double p0[3], const double p1[3], const double p2[3]) {
    const double k1x = p0[0] - p1[0], k1y = p0[1] - p1[1], k1z = p0[2] - p1[2];
    const double k2x = p0[0] - p2[0], k2y = p0[1] - p2[1], k2z = p0[2] - p2[2];
    const double cx = k1y * k2z - k1z * k2y, cy = k1z * k2x - k1x * k2z, cz = k1x * k2y - k1y * k2x;
    const double sq = (cx * cx + cy * cy) + cz * cz;
    const double len = sqrt(sq);   // correctly rounded on both sides, like the division below
    gr_plane g;
    g.p[0] = p0[0]; g.p[1] = p0[1]; g.p[2] = p0[2];
    g.n[0] = cx / len; g.n[1] = cy / len; g.n[2] = cz / len;
    return g;
}

// clustering.py:68-69: |dot(point - p0, n)|.  THE distance of this file: the scoring pass and the final mask both call it, so a
// hypothesis's count is the popcount of its mask.  A NaN normal gives NaN, and `d < tau` is then false (clustering.py:70).
__host__ __device__ inline double pcr_ground_distance(double x, double y, double z, double px, double py, double pz, double nx, double ny,
                                                      double nz) {
    const double vx = x - px, vy = y - py, vz = z - pz;
    return fabs((vx * nx + vy * ny) + vz * nz);
}

// clustering.py:50,75-81 over the counts of all trials: the running best is replaced on a strictly larger count, and right after a
// replacement the loop breaks when best / n > ratio.  count_of(j) reads trial j's count (host: the caller's array; device: L2).
template <typename Load>
__host__ __device__ inline int ground_select_rule(Load count_of, int32_t n_hyp, int64_t n, double ratio, int32_t* best_hyp, int32_t* evaluated) {
    long long best_cnt = 0;
    int32_t best = -1, ran = n_hyp;
    for (int32_t j = 0; j < n_hyp; ++j) {
        const long long c = count_of(j);
        if (c > best_cnt) {
            best_cnt = c;
            best = j;
            if ((double)best_cnt / (double)n > ratio) { ran = j + 1; break; }
        }
    }
    *best_hyp = best;
    *evaluated = ran;
    return best < 0 ? PCR_E_TOO_FEW_ASSOC : PCR_OK;   // every hypothesis degenerate: the reference indexes with None (clustering.py:83)
}

// slot_u[3h + s]: which distinct sampled row trial h's sample s is.  uxyz != null: the gathered points; else position = row.
__global__ void __launch_bounds__(GR_BLOCK)
ground_setup_kernel(const pcr_pt* __restrict__ pts, const double* __restrict__ uxyz, const long long* __restrict__ urows, const int* __restrict__ slot_u,
                    int n_hyp, gr_plane* __restrict__ planes, unsigned long long* __restrict__ counts, gr_state* __restrict__ st) {
    const int h = blockIdx.x * GR_BLOCK + threadIdx.x;
    if (h == 0) {
        st->best_hyp = -1; st->evaluated = 0; st->status = PCR_E_TOO_FEW_ASSOC; st->pad = 0;
        st->n_inliers = 0; st->n_outliers = 0; st->scan_total = 0;
    }
    if (h >= n_hyp) return;
    double p[3][3];
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        const int u = slot_u[3 * h + s];
        if (uxyz) { p[s][0] = uxyz[3 * u]; p[s][1] = uxyz[3 * u + 1]; p[s][2] = uxyz[3 * u + 2]; }
        else { const pcr_pt r = pts[urows[u]]; p[s][0] = r.x; p[s][1] = r.y; p[s][2] = r.z; }
    }
    planes[h] = pcr_ground_plane_from(p[0], p[1], p[2]);
    counts[h] = 0ull;
}

// Scores hypotheses h0 .. h0 + nh (nh <= GR_CHUNK) against every point.  A block takes GR_PTS * 256 points, GR_PTS per lane, held in
// registers while the chunk's planes go by, broadcast from LDS; a hypothesis's count over a wave's points is the popcount of the wave's
// ballots -- the same in every lane, scalar arithmetic, no reduction across the wave -- added to the block's counter in LDS by one lane.
__global__ void __launch_bounds__(GR_BLOCK)
ground_score_kernel(const pcr_pt* __restrict__ pts, long long n, const gr_plane* __restrict__ planes, int h0, int nh, double tau,
                    unsigned long long* __restrict__ counts, unsigned int* __restrict__ ticket, int last_chunk, int n_hyp, double ratio,
                    gr_state* __restrict__ st) {
    __shared__ double s_plane[GR_CHUNK][6];
    __shared__ unsigned int s_cnt[GR_CHUNK];
    __shared__ int s_last;
    for (int t = threadIdx.x; t < nh * 6; t += GR_BLOCK) {
        const gr_plane& g = planes[h0 + t / 6];
        const int k = t % 6;
        s_plane[t / 6][k] = k < 3 ? g.p[k] : g.n[k - 3];
    }
    for (int t = threadIdx.x; t < nh; t += GR_BLOCK) s_cnt[t] = 0u;
    double x[GR_PTS], y[GR_PTS], z[GR_PTS];
    bool valid[GR_PTS];
    block_tile_load<GR_PTS, false>(pts, n, x, y, z, valid, nullptr);
    __syncthreads();
    const bool first_lane = (threadIdx.x & 63) == 0;
    for (int h = 0; h < nh; ++h) {
        const double px = s_plane[h][0], py = s_plane[h][1], pz = s_plane[h][2], nx = s_plane[h][3], ny = s_plane[h][4], nz = s_plane[h][5];
        unsigned int c = 0u;
#pragma unroll
        for (int k = 0; k < GR_PTS; ++k) {
            const double d = pcr_ground_distance(x[k], y[k], z[k], px, py, pz, nx, ny, nz);
            c += (unsigned int)__popcll(__ballot(valid[k] && d < tau));
        }
        if (first_lane && c) atomicAdd(&s_cnt[h], c);
    }
    __syncthreads();
    // one device-scope add per hypothesis per block.  (Waves 1.. of a chunk of more than 64 hypotheses add too; the wait below and the
    // barrier behind it order every wave's adds in front of the ticket.)
    for (int t = threadIdx.x; t < nh; t += GR_BLOCK) {
        const unsigned long long v = s_cnt[t];
        if (v) __hip_atomic_fetch_add(&counts[h0 + t], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (!last_chunk) return;
    // The ticket of expand_cloud_kernel (pcr_core.hip): the adds above are device-scope atomics, performed at the coherence point and
    // acknowledged (vmcnt) before the block takes the ticket; no release fence, which is an L2 write-back on this chip.  The block
    // that arrives last reads the counts back with device-scope atomic loads.  Counts of earlier chunks are behind a kernel boundary.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned int t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = t == gridDim.x - 1u ? 1 : 0;
    }
    __syncthreads();
    if (!s_last || threadIdx.x != 0) return;
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next call (stream-ordered)
    int32_t best = -1, ran = 0;
    const int rc = ground_select_rule(
        [counts](int32_t j) { return (long long)__hip_atomic_load(&counts[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }, n_hyp, (int64_t)n, ratio,
        &best, &ran);
    st->best_hyp = best;
    st->evaluated = ran;
    st->status = rc;
    if (best >= 0) {
        const long long c = (long long)__hip_atomic_load(&counts[best], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        st->n_inliers = c;
        st->n_outliers = n - c;
        st->plane = planes[best];
    }
}

// flag[row] = 1 for an inlier of the winner, by CALLER row (the records may be Morton-reordered: id is the row)
__global__ void __launch_bounds__(GR_BLOCK)
ground_mask_kernel(const pcr_pt* __restrict__ pts, long long n, double tau, const gr_state* __restrict__ st, unsigned char* __restrict__ flag) {
    const long long i = (long long)blockIdx.x * GR_BLOCK + threadIdx.x;
    if (i >= n || st->best_hyp < 0) return;
    const gr_plane g = st->plane;
    const pcr_pt p = pts[i];
    const double d = pcr_ground_distance(p.x, p.y, p.z, g.p[0], g.p[1], g.p[2], g.n[0], g.n[1], g.n[2]);
    flag[p.id] = d < tau ? 1 : 0;
}

// Block scan over GR_TILE rows: pre[row] = outliers among the tile's rows in front of `row`, tile_sum[b] = outliers of tile b.
__global__ void __launch_bounds__(GR_BLOCK)
ground_scan_kernel(const unsigned char* __restrict__ flag, long long n, const gr_state* __restrict__ st, unsigned int* __restrict__ pre,
                   unsigned int* __restrict__ tile_sum) {
    __shared__ unsigned int s_wave[GR_BLOCK / 64];
    if (st->best_hyp < 0) return;
    const long long r0 = (long long)blockIdx.x * GR_TILE + 4ll * threadIdx.x;
    unsigned int o[4], mine = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        o[k] = (r0 + k < n && flag[r0 + k] == 0) ? 1u : 0u;
        mine += o[k];
    }
    const unsigned int inc = wave_incl_scan_add(mine);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    unsigned int before = inc - mine;
    for (int w = 0; w < wave; ++w) before += s_wave[w];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (r0 + k < n) pre[r0 + k] = before;
        before += o[k];
    }
    if (threadIdx.x == GR_BLOCK - 1) tile_sum[blockIdx.x] = before;
}

// exclusive scan of the tile sums in place (one block, tiles in order), total -> st->scan_total
__global__ void __launch_bounds__(GR_BLOCK)
ground_offsets_kernel(unsigned int* __restrict__ tile_sum, long long n_tiles, gr_state* __restrict__ st) {
    __shared__ unsigned int s_wave[GR_BLOCK / 64];
    __shared__ unsigned long long s_carry;
    if (st->best_hyp < 0) return;
    if (threadIdx.x == 0) s_carry = 0ull;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long long base = 0; base < n_tiles; base += GR_BLOCK) {
        const long long t = base + threadIdx.x;
        const unsigned int mine = t < n_tiles ? tile_sum[t] : 0u;
        const unsigned int inc = wave_incl_scan_add(mine);
        if (lane == 63) s_wave[wave] = inc;
        __syncthreads();
        unsigned long long before = s_carry + (inc - mine);
        for (int w = 0; w < wave; ++w) before += s_wave[w];
        if (t < n_tiles) tile_sum[t] = (unsigned int)before;
        __syncthreads();
        if (threadIdx.x == GR_BLOCK - 1) s_carry = before + mine;
        __syncthreads();
    }
    if (threadIdx.x == 0) st->scan_total = (long long)s_carry;
}

// outlier records to their rank among the outlier rows: a new cloud in ascending caller-row order with ids 0 .. m - 1, and the kept rows
__global__ void __launch_bounds__(GR_BLOCK)
ground_scatter_kernel(const pcr_pt* __restrict__ pts, long long n, const unsigned char* __restrict__ flag, const unsigned int* __restrict__ pre,
                      const unsigned int* __restrict__ tile_off, long long m, pcr_pt* __restrict__ out, int* __restrict__ rows_out) {
    const long long i = (long long)blockIdx.x * GR_BLOCK + threadIdx.x;
    if (i >= n) return;
    pcr_pt p = pts[i];
    const long long row = p.id;
    if (flag[row]) return;
    const long long dst = (long long)tile_off[row / GR_TILE] + pre[row];
    if (dst >= m) return;   // (cannot happen: m is the count of this very mask)
    if (rows_out) rows_out[dst] = (int)row;
    if (out) { p.id = dst; out[dst] = p; }
}

}  // namespace

extern "C" {

void pcr_ground_default_params(pcr_ground_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->tau = 0.6;     // clustering.py:17
    p->ratio = 0.5;   // clustering.py:19
    p->n_hyp = 35;    // clustering.py:18
}

int pcr_ground_select(const int64_t* counts, int32_t n_hyp, int64_t n, double ratio, int32_t* best_hyp, int32_t* evaluated) {
    if (!counts || !best_hyp || !evaluated || n_hyp < 1 || n < 1) return PCR_E_INVALID;
    for (int32_t j = 0; j < n_hyp; ++j)
        if (counts[j] < 0 || counts[j] > n) return PCR_E_INVALID;
    return ground_select_rule([counts](int32_t j) { return (long long)counts[j]; }, n_hyp, n, ratio, best_hyp, evaluated);
}

int pcr_ground_segmentation(pcr_ctx* ctx, const pcr_cloud* cloud, const int64_t* samples, const pcr_ground_params* params, pcr_cloud** outliers_out,
                            int32_t* outlier_rows_out, uint8_t* inlier_mask_out, int64_t* counts_out, pcr_ground_result* result) try {
    if (outliers_out) *outliers_out = nullptr;
    if (!ctx || !cloud || !samples || !params || !result) return PCR_E_INVALID;
    if (!std::isfinite(params->tau) || params->n_hyp < 1) return PCR_E_INVALID;
    const long long n = cloud->n;
    if (n <= 0) return PCR_E_EMPTY;
    const int n_hyp = params->n_hyp;
    const size_t n_slots = 3 * (size_t)n_hyp;
    for (size_t s = 0; s < n_slots; ++s)
        if (samples[s] < 0 || samples[s] >= n) return PCR_E_INVALID;
    hipSetDevice(ctx->device);
    memset(result, 0, sizeof(*result));
    result->best_hyp = -1;

    // distinct sampled rows, ascending, and for every sample slot its place among them
    std::vector<long long> urows(samples, samples + n_slots);
    std::sort(urows.begin(), urows.end());
    urows.erase(std::unique(urows.begin(), urows.end()), urows.end());
    const int nu = (int)urows.size();
    std::vector<int> slot_u(n_slots);
    for (size_t s = 0; s < n_slots; ++s) slot_u[s] = (int)(std::lower_bound(urows.begin(), urows.end(), (long long)samples[s]) - urows.begin());

    const long long n_tiles = (n + GR_TILE - 1) / GR_TILE;
    const bool want_compact = outliers_out || outlier_rows_out;
    pcr_dev_block b_urows(ctx), b_slot(ctx), b_uxyz(ctx), b_planes(ctx), b_counts(ctx), b_state(ctx), b_flag(ctx), b_pre(ctx), b_tiles(ctx), b_rows(ctx);
    int rc;
    if ((rc = b_urows.alloc(sizeof(long long) * nu)) || (rc = b_slot.alloc(sizeof(int) * n_slots)) || (rc = b_planes.alloc(sizeof(gr_plane) * n_hyp)) ||
        (rc = b_counts.alloc(sizeof(unsigned long long) * n_hyp)) || (rc = b_state.alloc(sizeof(gr_state))) || (rc = b_flag.alloc((size_t)n)))
        return rc;
    if (cloud->morton_sorted && (rc = b_uxyz.alloc(sizeof(double) * 3 * nu))) return rc;
    if (want_compact && ((rc = b_pre.alloc(sizeof(unsigned int) * n)) || (rc = b_tiles.alloc(sizeof(unsigned int) * n_tiles)))) return rc;
    PCR_HIP(ctx, hipMemcpyAsync(b_urows.p, urows.data(), sizeof(long long) * nu, hipMemcpyHostToDevice, ctx->stream));
    PCR_HIP(ctx, hipMemcpyAsync(b_slot.p, slot_u.data(), sizeof(int) * n_slots, hipMemcpyHostToDevice, ctx->stream));

    const pcr_pt* pts = cloud->d;
    gr_state* d_st = b_state.as<gr_state>();
    unsigned long long* d_counts = b_counts.as<unsigned long long>();
    const unsigned int grid_n = (unsigned int)((n + GR_BLOCK - 1) / GR_BLOCK);
    if (cloud->morton_sorted && (rc = pcr_cloud_gather_rows(ctx, cloud, b_urows.as<const long long>(), nullptr, nu, b_uxyz.as<double>()))) return rc;
    hipLaunchKernelGGL(ground_setup_kernel, dim3((unsigned int)((n_hyp + GR_BLOCK - 1) / GR_BLOCK)), dim3(GR_BLOCK), 0, ctx->stream, pts,
                       (const double*)b_uxyz.p, b_urows.as<const long long>(), b_slot.as<const int>(), n_hyp, b_planes.as<gr_plane>(), d_counts, d_st);
    PCR_HIP(ctx, hipGetLastError());
    const unsigned int grid_score = (unsigned int)((n + GR_PTS * GR_BLOCK - 1) / (GR_PTS * GR_BLOCK));
    for (int h0 = 0; h0 < n_hyp; h0 += GR_CHUNK) {
        const int nh = std::min(GR_CHUNK, n_hyp - h0);
        hipLaunchKernelGGL(ground_score_kernel, dim3(grid_score), dim3(GR_BLOCK), 0, ctx->stream, pts, n, b_planes.as<const gr_plane>(), h0, nh, params->tau,
                           d_counts, pcr_counter(ctx, PCR_CW_GROUND_TICKET), h0 + nh >= n_hyp ? 1 : 0, n_hyp, params->ratio, d_st);
        PCR_HIP(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(ground_mask_kernel, dim3(grid_n), dim3(GR_BLOCK), 0, ctx->stream, pts, n, params->tau, (const gr_state*)d_st, b_flag.as<unsigned char>());
    PCR_HIP(ctx, hipGetLastError());
    if (want_compact) {
        hipLaunchKernelGGL(ground_scan_kernel, dim3((unsigned int)n_tiles), dim3(GR_BLOCK), 0, ctx->stream, b_flag.as<const unsigned char>(), n, (const gr_state*)d_st,
                           b_pre.as<unsigned int>(), b_tiles.as<unsigned int>());
        PCR_HIP(ctx, hipGetLastError());
        hipLaunchKernelGGL(ground_offsets_kernel, dim3(1), dim3(GR_BLOCK), 0, ctx->stream, b_tiles.as<unsigned int>(), n_tiles, d_st);
        PCR_HIP(ctx, hipGetLastError());
    }
    // the only read-back the step needs: the winner and its counts (the size of the new cloud is a host-side field)
    gr_state h_st;
    if ((rc = pcr_d2h_small(ctx, &h_st, d_st, sizeof(h_st)))) return rc;
    result->best_hyp = h_st.best_hyp;
    result->evaluated = h_st.evaluated;
    if (counts_out) {
        PCR_HIP(ctx, hipMemcpyAsync(counts_out, d_counts, sizeof(int64_t) * n_hyp, hipMemcpyDeviceToHost, ctx->stream));
        PCR_HIP(ctx, pcr_sync(ctx->stream));
    }
    if (h_st.status != PCR_OK) return h_st.status;
    result->n_inliers = h_st.n_inliers;
    result->n_outliers = h_st.n_outliers;
    for (int k = 0; k < 3; ++k) { result->point[k] = h_st.plane.p[k]; result->normal[k] = h_st.plane.n[k]; }
    const long long m = h_st.n_outliers;
    if (want_compact && h_st.scan_total != m) {
        ctx->last_error = "pcr_ground_segmentation: the mask of the winning hypothesis does not match its count";
        return PCR_E_HIP;
    }
    if (inlier_mask_out) PCR_HIP(ctx, hipMemcpyAsync(inlier_mask_out, b_flag.p, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    pcr_cloud_guard c(ctx);
    if (want_compact) {
        if (outliers_out) {
            c.h = new pcr_cloud();
            c->n = m;
            if ((rc = pcr_dev_alloc(ctx, sizeof(pcr_pt) * m, (void**)&c->d))) return rc;
        }
        if (outlier_rows_out && (rc = b_rows.alloc(sizeof(int) * m))) return rc;
        if (m > 0) {
            hipLaunchKernelGGL(ground_scatter_kernel, dim3(grid_n), dim3(GR_BLOCK), 0, ctx->stream, pts, n, b_flag.as<const unsigned char>(), b_pre.as<const unsigned int>(),
                               b_tiles.as<const unsigned int>(), m, c.h ? c->d : (pcr_pt*)nullptr, outlier_rows_out ? b_rows.as<int>() : (int*)nullptr);
            PCR_HIP(ctx, hipGetLastError());
            if (outlier_rows_out) PCR_HIP(ctx, hipMemcpyAsync(outlier_rows_out, b_rows.p, sizeof(int) * m, hipMemcpyDeviceToHost, ctx->stream));
        }
    }
    if (inlier_mask_out || outlier_rows_out) PCR_HIP(ctx, pcr_sync(ctx->stream));   // host buffers are only written during the call
    if (outliers_out) *outliers_out = c.release();
    return PCR_OK;
} PCR_CATCH(ctx)

}  // extern "C"
