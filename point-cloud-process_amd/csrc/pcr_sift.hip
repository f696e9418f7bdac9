// SIFT-3D keypoints -- the scale-space detector of PCLKeypoints/src/keypoints.cpp (keypointSift: pcl::SIFTKeypoint on the y coordinate),
// by the rules stated in include/pcr.h (PCL itself is not part of the build: parity with its binary32 output is unpinned).  Per octave:
//   DoG        the wave walk of pcr_ball_visit.h (one wave per point) over the ball of 3 sigma_max: per scale a Gaussian-weighted mean of
//              the field, 2 S accumulators in registers (S padded to 8 or 16 by the template: no array indexed at run time); a neighbour
//              enters at the first scale whose limit holds it and at every scale after it.  D = differences of adjacent scales, by row.
//              (Measured against the lane-group walk, 8 lanes per point: the wave is 1.1-2.2 x faster at balls of 44-90 rows and 2.1-3.0 x
//              at 290-900, DESIGN.md section 3.4.2 -- a lane of a group walks whole cells on its own, and the binary64 exp of up to 16
//              scales per record wants all the lanes it can get.)  A sum's order: lane l takes the records l, l + 64, ... of the 27 runs
//              in turn, then the lanes by wave_sum_all.
//   flags      one per row: some interior column passes the contrast test and the strict test against its own two adjacent columns;
//              rocprim::select over the row numbers follows, so candidates are in ascending caller row
//   extrema    one wave per candidate: ONE pass over the 27-cell block stages the ball's (d2, row) pairs in LDS; the 25 rows smallest in
//              (d2, row) are a set: an LDS histogram of d2 finds the bin of the 25th pair (pcr_shot.hip's technique), every pair below it is
//              in, and selection rounds ("the least above the last", k-NN's rule) settle the threshold bin alone; then sift_compare.  A
//              candidate whose ball holds fewer rows than that (or more than the stage) goes onto a list: knn_kernel (its list mode, the
//              exact descent) finds its rows and sift_compare_kernel runs the same comparison.  One mask of kept columns per candidate.
//   entries    popcounts of the masks, an exclusive scan, one store per entry in (row, column) order
// Nothing adds with atomics (the list counter is an integer), every sum runs in a fixed order, and the host waits once per octave, for the
// number of entries (beside the waits of the voxel filter and the grid build); pcr_sift keeps every octave's keypoints on the device and
// downloads them once behind the loop.
#include <cfloat>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include "pcr_ball_visit.h"
#include "pcr_sort.h"

constexpr int SIFT_NN = 25;       // rows of N(i)
constexpr int SIFT_MAX_S = 16;    // scales of an octave: q + 3, q <= 13

struct sift_tables {   // lim = 9 sigma^2, h = -0.5 / sigma^2 per scale; lim = -1 past the last scale (no d2 is inside)
    double lim[SIFT_MAX_S], h[SIFT_MAX_S], sigma[SIFT_MAX_S];
};

template <int SP>
__global__ void __launch_bounds__(256) sift_dog_kernel(pcr_grid_view gv, long long n, sift_tables t, int S, double lim_max, int field,
                                                       double* __restrict__ D /* by row (n, S - 1) */, int* __restrict__ counts /* by row */) {
    const int lane = threadIdx.x & 63;
    const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const pcr_pt p = gv.pts[i];
    double num[SP], den[SP];
#pragma unroll
    for (int s = 0; s < SP; ++s) num[s] = den[s] = 0.0;
    int c = 0;
    auto f = [&](unsigned int j, bool valid) {
        if (!valid) return;
        const pcr_pt b = gv.pts[j];
        const double d2 = dist2(p.x, p.y, p.z, b);
        if (d2 <= lim_max) {
            ++c;
            const double v = field == 0 ? b.x : (field == 1 ? b.y : b.z);
#pragma unroll
            for (int s = 0; s < SP; ++s)
                if (d2 <= t.lim[s]) {
                    const double w = exp(d2 * t.h[s]);
                    num[s] += v * w;
                    den[s] += w;
                }
        }
    };
    unsigned int rs, re;
    wave_block_runs(gv, p.x, p.y, p.z, lane, &rs, &re);
    wave_visit_runs(rs, re, lane, f);
#pragma unroll
    for (int s = 0; s < SP; ++s) {
        num[s] = wave_sum_all(num[s]);
        den[s] = wave_sum_all(den[s]);
    }
    c = wave_sum_all(c);
    if (lane != 0) return;
    counts[p.id] = c;
    double* out = D + p.id * (S - 1);
#pragma unroll
    for (int s = 0; s + 1 < SP; ++s)
        if (s + 1 < S) out[s] = num[s + 1] / den[s + 1] - num[s] / den[s];
}

__global__ void sift_row_pos_kernel(const pcr_pt* __restrict__ pts, long long n, unsigned int* __restrict__ row_pos /* by row */) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) row_pos[pts[i].id] = (unsigned int)i;
}

// a row is a candidate iff some interior column passes the contrast test and is strictly below or strictly above both adjacent columns
__device__ static inline bool sift_own_columns(double val, double lo, double hi, double contrast, bool* is_min) {
    if (!(fabs(val) >= contrast)) return false;
    *is_min = val < lo && val < hi;
    return *is_min || (val > lo && val > hi);
}
__global__ void sift_flag_kernel(const double* __restrict__ D, long long n, int C, double contrast, unsigned char* __restrict__ flags) {
    const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n) return;
    const double* d = D + row * C;
    bool any = false, is_min;
    for (int c = 1; c + 1 < C; ++c) any = any || sift_own_columns(d[c], d[c - 1], d[c + 1], contrast, &is_min);
    flags[row] = any ? 1 : 0;
}

// THE comparison, by a whole wave: lane l holds row `nb` of N(row) when `has`.  -> the columns c (bit c) at which (row, c) is a keypoint:
// a minimum that no value of the neighbours' columns c - 1, c, c + 1 is below, or the mirrored maximum.  Ties with a neighbour keep it.
__device__ static inline unsigned int sift_compare(const double* __restrict__ D, int C, double contrast, long long row, long long nb, bool has) {
    const double* d = D + row * C;
    const double* o = D + (has ? nb : row) * C;
    unsigned int mask = 0;
    for (int c = 1; c + 1 < C; ++c) {   // (wave-uniform: every lane reads the same row)
        const double val = d[c];
        bool is_min;
        if (!sift_own_columns(val, d[c - 1], d[c + 1], contrast, &is_min)) continue;
        bool beaten = false;
        if (has)
            for (int e = c - 1; e <= c + 1; ++e) beaten = beaten || (is_min ? val > o[e] : val < o[e]);
        if (__ballot(beaten) == 0ull) mask |= 1u << c;
    }
    return mask;
}

// One wave per candidate, two to a block.  k = min(25, n).  When the ball holds >= k rows, the k rows smallest in (d2, row) of the ball are
// those of the whole cloud.  ONE pass over the 27 runs stages the ball's (d2, row) pairs in LDS (ballot compaction, in walk order); the
// ranking then reads LDS only: a 256-bin histogram of d2 finds the bin of the k-th pair, selection rounds settle that bin alone.  (The
// first form ran 25 selection rounds over the 27 runs in global memory: 25 x 27 dependent loads a candidate, pure latency; the second ran
// the 25 rounds over LDS -- DESIGN.md section 3.4.2 has the three measured.)
// A ball of fewer than k rows, or of more than SIFT_STAGE, goes onto the list.
constexpr int SIFT_STAGE = 2048;   // staged pairs per wave: 24 KiB
constexpr int SIFT_BINS = 256;     // of the d2 histogram: four to a lane
constexpr int SIFT_SEL = 32;       // >= SIFT_NN
__global__ void __launch_bounds__(128) sift_extrema_kernel(pcr_grid_view gv, const int* __restrict__ cand, const unsigned int* __restrict__ n_cand,
                                                           const unsigned int* __restrict__ row_pos, double r2_in, int k, const double* __restrict__ D, int C,
                                                           double contrast, unsigned int* __restrict__ masks /* by candidate */, int* __restrict__ list,
                                                           unsigned int* __restrict__ list_count, double* __restrict__ list_q /* 3 per candidate */) {
    __shared__ double s_d2[2][SIFT_STAGE];
    __shared__ int s_id[2][SIFT_STAGE];
    __shared__ unsigned int s_hist[2][SIFT_BINS];
    __shared__ int s_sel[2][SIFT_SEL];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned int slot = blockIdx.x * 2u + wave;
    if (slot >= *n_cand) return;   // (the whole wave; nothing below waits for the other wave)
    const long long row = cand[slot];
    const pcr_pt p = gv.pts[row_pos[row]];
    unsigned int s, e;
    wave_block_runs(gv, p.x, p.y, p.z, lane, &s, &e);
    int in_ball = 0;
    auto f = [&](unsigned int j, bool valid) {
        double d2 = 0.0;
        int id = 0;
        bool in = false;
        if (valid) {
            const pcr_pt b = gv.pts[j];
            d2 = dist2(p.x, p.y, p.z, b);
            id = (int)b.id;
            in = d2 <= r2_in;
        }
        int added;
        const int at = in_ball + wave_compact_slot(in, lane, &added);
        if (in && at < SIFT_STAGE) {
            s_d2[wave][at] = d2;
            s_id[wave][at] = id;
        }
        in_ball += added;
    };
    wave_visit_runs(s, e, lane, f);
    if (in_ball < k || in_ball > SIFT_STAGE) {   // (also a centre whose cell was clamped: it met no record)
        if (lane == 0) {
            const unsigned int at = atomicAdd(list_count, 1u);
            list[at] = (int)slot;
            list_q[3 * slot + 0] = p.x;
            list_q[3 * slot + 1] = p.y;
            list_q[3 * slot + 2] = p.z;
        }
        return;
    }
    // N(row) is a SET: the k smallest in (d2, row).  A histogram of d2 over the ball's range finds the bin that holds the k-th (pcr_shot.hip's
    // technique): every pair in a lower bin is in, and of the threshold bin the `need` smallest, found by `need` selection rounds.
    wave_sync();
    unsigned int* const hist = s_hist[wave];
    for (int b = lane; b < SIFT_BINS; b += 64) hist[b] = 0u;
    wave_sync();
    const double to_bin = (double)SIFT_BINS / r2_in;
    auto bin_of = [&](double d2) {   // (monotone in d2)
        const int b = (int)(d2 * to_bin);
        return b < SIFT_BINS ? b : SIFT_BINS - 1;
    };
    for (int j = lane; j < in_ball; j += 64) atomicAdd(&hist[bin_of(s_d2[wave][j])], 1u);
    wave_sync();
    unsigned int h[4], own = 0u;   // lane l owns the bins 4 l .. 4 l + 3
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        h[u] = hist[4 * lane + u];
        own += h[u];
    }
    unsigned int incl = own;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned int t = __shfl_up(incl, off, 64);
        if (lane >= off) incl += t;
    }
    const unsigned int excl = incl - own, ku = (unsigned int)k;
    const bool here = excl < ku && ku <= incl;   // (one lane: the counts end at in_ball >= k)
    int T = 0;
    unsigned int below = excl;
    if (here) {
        bool found = false;
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (!found) {
                if (below + h[u] >= ku) { T = 4 * lane + u; found = true; }
                else below += h[u];
            }
    }
    const int src = __ffsll((unsigned long long)__ballot(here)) - 1;
    T = __shfl(T, src, 64);
    below = __shfl(below, src, 64);
    const int need = k - (int)below;   // >= 1 pairs of bin T
    double cut_d2 = -1.0;
    long long cut_id = -1;
    for (int r = 0; r < need; ++r) {
        double bd2 = DBL_MAX;
        long long bid = 0x7fffffffffffffffll;
        for (int j = lane; j < in_ball; j += 64) {
            const double d2 = s_d2[wave][j];
            const long long id = s_id[wave][j];
            const bool above = d2 > cut_d2 || (d2 == cut_d2 && id > cut_id);
            if (bin_of(d2) == T && above && better(d2, id, bd2, bid)) { bd2 = d2; bid = id; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double od2 = __shfl_xor(bd2, off, 64);
            const long long oid = __shfl_xor(bid, off, 64);
            if (better(od2, oid, bd2, bid)) { bd2 = od2; bid = oid; }
        }
        cut_d2 = bd2;
        cut_id = bid;
    }
    int base = 0;   // the members, one to a lane, in staged order
    for (int j0 = 0; j0 < in_ball; j0 += 64) {
        const int j = j0 + lane;
        bool in = false;
        int id = 0;
        if (j < in_ball) {
            const double d2 = s_d2[wave][j];
            id = s_id[wave][j];
            const int b = bin_of(d2);
            in = b < T || (b == T && !(d2 > cut_d2 || (d2 == cut_d2 && id > cut_id)));
        }
        int added;
        const int at = base + wave_compact_slot(in, lane, &added);
        if (in && at < SIFT_SEL) s_sel[wave][at] = id;
        base += added;
    }
    wave_sync();
    const long long mine = lane < k ? s_sel[wave][lane] : -1;
    const unsigned int mask = sift_compare(D, C, contrast, row, mine, lane < k);
    if (lane == 0) masks[slot] = mask;
}

// the candidates of the list, their k rows found by knn_kernel at nbr[slot * k ...]
__global__ void __launch_bounds__(256) sift_compare_kernel(const int* __restrict__ cand, const int* __restrict__ list, const unsigned int* __restrict__ list_count,
                                                           const int* __restrict__ nbr, int k, const double* __restrict__ D, int C, double contrast,
                                                           unsigned int* __restrict__ masks) {
    const int lane = threadIdx.x & 63;
    const unsigned int at = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (at >= *list_count) return;
    const long long slot = list[at];
    const long long nb = lane < k ? nbr[slot * k + lane] : -1;
    const unsigned int mask = sift_compare(D, C, contrast, cand[slot], nb, lane < k);
    if (lane == 0) masks[slot] = mask;
}

struct sift_popc {
    __host__ __device__ unsigned int operator()(unsigned int m) const {
#if defined(__HIP_DEVICE_COMPILE__)
        return (unsigned int)__popc(m);
#else
        return (unsigned int)__builtin_popcount(m);
#endif
    }
};
__global__ void sift_total_kernel(const unsigned int* __restrict__ masks, const unsigned int* __restrict__ offs, long long n, unsigned int* __restrict__ total) {
    *total = offs[n - 1] + sift_popc()(masks[n - 1]);
}
__global__ void sift_entries_kernel(const unsigned int* __restrict__ masks, const unsigned int* __restrict__ offs, const int* __restrict__ cand, long long n,
                                    int* __restrict__ rows, int* __restrict__ cols) {
    const long long slot = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= n) return;
    unsigned int m = masks[slot], o = offs[slot];
    while (m) {
        rows[o] = cand[slot];
        cols[o] = __ffs(m) - 1;
        ++o;
        m &= m - 1u;
    }
}
__global__ void sift_keypoints_kernel(const pcr_pt* __restrict__ pts, const unsigned int* __restrict__ row_pos, const int* __restrict__ rows, const int* __restrict__ cols,
                                      unsigned int m, sift_tables t, double* __restrict__ out /* (m, 5): x, y, z, scale, row */) {
    const unsigned int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const pcr_pt p = pts[row_pos[rows[j]]];
    out[5 * j + 0] = p.x;
    out[5 * j + 1] = p.y;
    out[5 * j + 2] = p.z;
    out[5 * j + 3] = t.sigma[cols[j]];
    out[5 * j + 4] = (double)rows[j];
}

// what one octave leaves on the device
struct sift_stage {
    pcr_index_guard idx;
    pcr_dev_block D, counts, row_pos, rows, cols;
    unsigned int k = 0;   // entries
    explicit sift_stage(pcr_ctx* ctx) : idx(ctx), D(ctx), counts(ctx), row_pos(ctx), rows(ctx), cols(ctx) {}
};

// the extrema of the table st.D (n x C, by row) over the grid st.idx whose block covers the ball of squared radius r2_in: entries -> st.rows /
// st.cols (ascending (row, column)), their number -> st.k.  Waits for the device once.
static int sift_extrema_stage(pcr_ctx* ctx, sift_stage& st, int64_t n, int C, double contrast, double r2_in, const char* who) {
    const pcr_grid_view& gv = st.idx->view;
    const int k = n < SIFT_NN ? (int)n : SIFT_NN;
    const unsigned int waves = (unsigned int)((n + 3) / 4), threads = (unsigned int)((n + 255) / 256);
    pcr_dev_block b_flags(ctx), b_cand(ctx), b_words(ctx), b_tmp(ctx), b_masks(ctx), b_list(ctx), b_q(ctx), b_nbr(ctx), b_dist(ctx), b_offs(ctx), b_tmp2(ctx);
    int rc;
    if ((rc = b_flags.alloc((size_t)n)) || (rc = b_cand.alloc(sizeof(int) * n)) || (rc = b_words.alloc(4 * sizeof(unsigned int))) ||
        (rc = b_masks.alloc(sizeof(unsigned int) * n)) || (rc = b_list.alloc(sizeof(int) * n)) || (rc = b_q.alloc(sizeof(double) * 3 * n)) ||
        (rc = b_nbr.alloc(sizeof(int) * (size_t)k * n)) || (rc = b_dist.alloc(sizeof(double) * (size_t)k * n)) || (rc = b_offs.alloc(sizeof(unsigned int) * n)) ||
        (rc = st.row_pos.alloc(sizeof(unsigned int) * n)))
        return rc;
    unsigned int* const d_n_cand = b_words.as<unsigned int>();   // [0] candidates, [1] list length, [2] entries
    unsigned int* const d_masks = b_masks.as<unsigned int>();
    const double* const d_D = st.D.as<double>();
    PCR_HIP(ctx, hipMemsetAsync(d_n_cand, 0, 4 * sizeof(unsigned int), ctx->stream));
    PCR_HIP(ctx, hipMemsetAsync(d_masks, 0, sizeof(unsigned int) * (size_t)n, ctx->stream));
    hipLaunchKernelGGL(sift_row_pos_kernel, dim3(threads), dim3(256), 0, ctx->stream, gv.pts, (long long)n, st.row_pos.as<unsigned int>());
    hipLaunchKernelGGL(sift_flag_kernel, dim3(threads), dim3(256), 0, ctx->stream, d_D, (long long)n, C, contrast, b_flags.as<unsigned char>());
    PCR_HIP(ctx, hipGetLastError());
    if ((rc = pcr_select_positions(ctx, b_flags.as<unsigned char>(), (size_t)n, b_cand.as<int>(), d_n_cand, b_tmp, who))) return rc;
    // (the grids cover every row: the candidates' number is only known on the device)
    hipLaunchKernelGGL(sift_extrema_kernel, dim3((unsigned int)((n + 1) / 2)), dim3(128), 0, ctx->stream, gv, (const int*)b_cand.p, (const unsigned int*)d_n_cand,
                       (const unsigned int*)st.row_pos.p, r2_in, k, d_D, C, contrast, d_masks, b_list.as<int>(), d_n_cand + 1, b_q.as<double>());
    PCR_HIP(ctx, hipGetLastError());
    if ((rc = pcr_knn_list_dev(ctx, st.idx.h, b_q.as<double>(), n, k, b_nbr.as<int>(), b_dist.as<double>(), (const int*)b_list.p, (const unsigned int*)(d_n_cand + 1))))
        return rc;
    hipLaunchKernelGGL(sift_compare_kernel, dim3(waves), dim3(256), 0, ctx->stream, (const int*)b_cand.p, (const int*)b_list.p, (const unsigned int*)(d_n_cand + 1),
                       (const int*)b_nbr.p, k, d_D, C, contrast, d_masks);
    PCR_HIP(ctx, hipGetLastError());
    const auto popc = rocprim::make_transform_iterator((const unsigned int*)d_masks, sift_popc());
    size_t tmp_bytes = 0;
    hipError_t e = rocprim::exclusive_scan(nullptr, tmp_bytes, popc, b_offs.as<unsigned int>(), 0u, (size_t)n, rocprim::plus<unsigned int>(), ctx->stream);
    if (e == hipSuccess && (rc = b_tmp2.alloc(tmp_bytes ? tmp_bytes : 16)) == PCR_OK)
        e = rocprim::exclusive_scan(b_tmp2.p, tmp_bytes, popc, b_offs.as<unsigned int>(), 0u, (size_t)n, rocprim::plus<unsigned int>(), ctx->stream);
    if (rc) return rc;
    if (e != hipSuccess) {
        ctx->last_error = std::string(who) + " (scan): " + hipGetErrorString(e);
        return PCR_E_HIP;
    }
    hipLaunchKernelGGL(sift_total_kernel, dim3(1), dim3(1), 0, ctx->stream, (const unsigned int*)d_masks, (const unsigned int*)b_offs.p, (long long)n, d_n_cand + 2);
    PCR_HIP(ctx, hipGetLastError());
    if ((rc = pcr_d2h_small(ctx, &st.k, d_n_cand + 2, sizeof(unsigned int)))) return rc;   // THE wait of the octave
    if (st.k == 0) return PCR_OK;
    if ((rc = st.rows.alloc(sizeof(int) * st.k)) || (rc = st.cols.alloc(sizeof(int) * st.k))) return rc;
    hipLaunchKernelGGL(sift_entries_kernel, dim3(threads), dim3(256), 0, ctx->stream, (const unsigned int*)d_masks, (const unsigned int*)b_offs.p, (const int*)b_cand.p,
                       (long long)n, st.rows.as<int>(), st.cols.as<int>());
    PCR_HIP(ctx, hipGetLastError());
    return PCR_OK;   // (enqueued: the scratch of this scope goes back to the arena, whose next users are behind it on the stream)
}

static bool sift_q_ok(pcr_ctx* ctx, int q, const char* who) {
    if (q >= 1 && q + 3 <= SIFT_MAX_S) return true;
    if (ctx) ctx->last_error = std::string(who) + ": n_scales_per_octave = " + std::to_string(q) + ", supported are 1 .. 13 (at most 16 scales an octave)";
    return false;
}
static void sift_make_tables(double b, int q, sift_tables* t) {
    const int S = q + 3;
    for (int s = 0; s < SIFT_MAX_S; ++s) {
        t->sigma[s] = 0.0;
        t->lim[s] = -1.0;
        t->h[s] = 0.0;
    }
    for (int s = 0; s < S; ++s) {
        const double sigma = b * pow(2.0, (s - 1.0) / q), sigma2 = sigma * sigma;
        t->sigma[s] = sigma;
        t->lim[s] = 9.0 * sigma2;
        t->h[s] = -0.5 / sigma2;
    }
}

// one octave on the cloud as given: grid, DoG and, when entries are asked for, extrema.  st.D (n x C) and st.counts (n) by row.
static int sift_octave_stage(pcr_ctx* ctx, const pcr_cloud* cloud, int q, double contrast, int field, const sift_tables& t, sift_stage& st, bool want_entries,
                             const char* who) {
    const int64_t n = cloud->n;
    const int S = q + 3, C = q + 2;
    int rc = ball_grid(ctx, cloud, 3.0 * t.sigma[S - 1], who, st.idx);
    if (rc) return rc;
    if ((rc = st.D.alloc(sizeof(double) * (size_t)C * n)) || (rc = st.counts.alloc(sizeof(int) * n))) return rc;
    const unsigned waves = (unsigned)((n + 3) / 4);
    if (S <= 8)
        hipLaunchKernelGGL(sift_dog_kernel<8>, dim3(waves), dim3(256), 0, ctx->stream, st.idx->view, (long long)n, t, S, t.lim[S - 1], field, st.D.as<double>(),
                           st.counts.as<int>());
    else
        hipLaunchKernelGGL(sift_dog_kernel<16>, dim3(waves), dim3(256), 0, ctx->stream, st.idx->view, (long long)n, t, S, t.lim[S - 1], field, st.D.as<double>(),
                           st.counts.as<int>());
    PCR_HIP(ctx, hipGetLastError());
    if (!want_entries) return PCR_OK;
    return sift_extrema_stage(ctx, st, n, C, contrast, t.lim[S - 1], who);
}

static int sift_capacity(pcr_ctx* ctx, const char* who, int64_t capacity, int64_t needed) {
    if (needed <= capacity) return PCR_OK;
    ctx->last_error = std::string(who) + ": the keypoint buffer holds " + std::to_string(capacity) + " entries, " + std::to_string(needed) + " are needed";
    return PCR_E_UNSUPPORTED;
}

extern "C" int pcr_sift_scales(double base_scale, int n_scales_per_octave, double* scales_out) {
    if (!scales_out || !(base_scale > 0) || !std::isfinite(base_scale)) return PCR_E_INVALID;
    if (!sift_q_ok(nullptr, n_scales_per_octave, "pcr_sift_scales")) return PCR_E_UNSUPPORTED;
    sift_tables t;
    sift_make_tables(base_scale, n_scales_per_octave, &t);
    memcpy(scales_out, t.sigma, sizeof(double) * (n_scales_per_octave + 3));
    return PCR_OK;
}

extern "C" int pcr_sift_octave(pcr_ctx* ctx, const pcr_cloud* cloud, double base_scale, int n_scales_per_octave, double min_contrast, int field, double* dog_out,
                               int32_t* counts_out, int32_t* rows_out, int32_t* cols_out, int64_t capacity, int64_t* n_out) try {
    if (!ctx || !cloud) return PCR_E_INVALID;
    if (!(base_scale > 0) || !std::isfinite(base_scale) || std::isnan(min_contrast) || min_contrast < 0 || field < 0 || field > 2) return PCR_E_INVALID;
    const bool want_kp = rows_out != nullptr;
    if (want_kp && (!cols_out || !n_out || capacity < 0)) return PCR_E_INVALID;
    if (!want_kp && (cols_out || (!dog_out && !counts_out))) return PCR_E_INVALID;   // columns without rows, or nothing asked for
    if (!sift_q_ok(ctx, n_scales_per_octave, "pcr_sift_octave")) return PCR_E_UNSUPPORTED;
    if (cloud->n <= 0) return PCR_E_EMPTY;
    hipSetDevice(ctx->device);
    const int64_t n = cloud->n;
    const int C = n_scales_per_octave + 2;
    sift_tables t;
    sift_make_tables(base_scale, n_scales_per_octave, &t);
    sift_stage st(ctx);
    int rc = sift_octave_stage(ctx, cloud, n_scales_per_octave, min_contrast, field, t, st, want_kp, "pcr_sift_octave");
    if (rc) return rc;
    // (the per-row results are the caller's even when the entry buffer was too small)
    if (dog_out && (rc = pcr_d2h_staged(ctx, dog_out, st.D.p, sizeof(double) * (size_t)C * n))) return rc;
    if (counts_out && (rc = pcr_d2h_staged(ctx, counts_out, st.counts.p, sizeof(int) * (size_t)n))) return rc;
    if (!want_kp) return PCR_OK;
    *n_out = (int64_t)st.k;
    if ((rc = sift_capacity(ctx, "pcr_sift_octave", capacity, st.k)) || st.k == 0) return rc;
    if ((rc = pcr_d2h_staged(ctx, rows_out, st.rows.p, sizeof(int) * (size_t)st.k))) return rc;
    return pcr_d2h_staged(ctx, cols_out, st.cols.p, sizeof(int) * (size_t)st.k);
} PCR_CATCH(ctx)

extern "C" int pcr_sift_extrema(pcr_ctx* ctx, const pcr_cloud* cloud, const double* dog, int n_columns, double min_contrast, int32_t* rows_out, int32_t* cols_out,
                                int64_t capacity, int64_t* n_out) try {
    if (!ctx || !cloud || !dog || !rows_out || !cols_out || !n_out || capacity < 0) return PCR_E_INVALID;
    if (std::isnan(min_contrast) || min_contrast < 0 || n_columns < 3) return PCR_E_INVALID;
    if (n_columns > SIFT_MAX_S - 1) {
        ctx->last_error = "pcr_sift_extrema: " + std::to_string(n_columns) + " columns, supported are 3 .. 15";
        return PCR_E_UNSUPPORTED;
    }
    if (cloud->n <= 0) return PCR_E_EMPTY;
    hipSetDevice(ctx->device);
    const int64_t n = cloud->n;
    // No scale comes with a table: the walk takes a ball that holds some hundred rows of an evenly filled box or sheet of the cloud's
    // extent.  N(i) does not depend on it -- a candidate whose ball holds fewer than 25 rows takes the list's way.
    double lo[3], hi[3];
    int rc = pcr_cloud_bbox(ctx, cloud, lo, hi);
    if (rc) return rc;
    double ext = 0.0;
    for (int a = 0; a < 3; ++a) ext = fmax(ext, hi[a] - lo[a]);
    double radius = ext * cbrt(32.0 / (double)n);
    if (!(radius > 0) || !std::isfinite(radius)) radius = 1.0;
    sift_stage st(ctx);
    if ((rc = ball_grid(ctx, cloud, radius, "pcr_sift_extrema", st.idx))) return rc;
    if ((rc = st.D.alloc(sizeof(double) * (size_t)n_columns * n))) return rc;
    PCR_HIP(ctx, hipMemcpyAsync(st.D.p, dog, sizeof(double) * (size_t)n_columns * n, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = sift_extrema_stage(ctx, st, n, n_columns, min_contrast, radius * radius, "pcr_sift_extrema"))) return rc;   // (waits: the caller's table is free)
    *n_out = (int64_t)st.k;
    if ((rc = sift_capacity(ctx, "pcr_sift_extrema", capacity, st.k)) || st.k == 0) return rc;
    if ((rc = pcr_d2h_staged(ctx, rows_out, st.rows.p, sizeof(int) * (size_t)st.k))) return rc;
    return pcr_d2h_staged(ctx, cols_out, st.cols.p, sizeof(int) * (size_t)st.k);
} PCR_CATCH(ctx)

extern "C" int pcr_sift(pcr_ctx* ctx, const pcr_cloud* cloud, double min_scale, int n_octaves, int n_scales_per_octave, double min_contrast, int field,
                        double* keypoints_out, int32_t* octave_out, int32_t* row_out, int64_t capacity, int64_t* n_out, int64_t* octave_sizes_out) try {
    if (!ctx || !cloud || !keypoints_out || !n_out || capacity < 0) return PCR_E_INVALID;
    if (n_octaves < 1 || !(min_scale > 0) || !std::isfinite(min_scale) || std::isnan(min_contrast) || min_contrast < 0 || field < 0 || field > 2) return PCR_E_INVALID;
    if (!sift_q_ok(ctx, n_scales_per_octave, "pcr_sift")) return PCR_E_UNSUPPORTED;
    if (cloud->n <= 0) return PCR_E_EMPTY;
    hipSetDevice(ctx->device);
    if (octave_sizes_out)
        for (int o = 0; o < n_octaves; ++o) octave_sizes_out[o] = 0;
    // every octave's keypoints stay on the device (5 doubles each: x, y, z, scale, row) and come down once, behind the loop
    struct kept { std::unique_ptr<pcr_dev_block> block; unsigned int k; int octave; };
    std::vector<kept> octaves;
    int64_t total = 0;
    double scale = min_scale;
    pcr_cloud_guard cur(ctx);
    const pcr_cloud* in = cloud;
    int rc;
    for (int o = 0; o < n_octaves; ++o, scale *= 2.0) {
        if (!std::isfinite(scale)) break;
        pcr_cloud* down = nullptr;
        if ((rc = pcr_voxel_filter_cloud(ctx, in, scale, 2, 0, &down))) return rc;
        pcr_cloud_guard next(ctx, down);
        const int64_t n = down->n;
        if (n < SIFT_NN) break;
        if (octave_sizes_out) octave_sizes_out[o] = n;
        sift_tables t;
        sift_make_tables(scale, n_scales_per_octave, &t);
        sift_stage st(ctx);
        if ((rc = sift_octave_stage(ctx, down, n_scales_per_octave, min_contrast, field, t, st, true, "pcr_sift"))) return rc;   // (its one wait: st.k)
        total += st.k;
        if (st.k && total <= capacity) {   // (past the capacity only the count goes on)
            octaves.push_back(kept{std::make_unique<pcr_dev_block>(ctx), st.k, o});
            pcr_dev_block& b_kp = *octaves.back().block;
            if ((rc = b_kp.alloc(sizeof(double) * 5 * st.k))) return rc;
            hipLaunchKernelGGL(sift_keypoints_kernel, dim3((st.k + 255) / 256), dim3(256), 0, ctx->stream, st.idx->view.pts, (const unsigned int*)st.row_pos.p,
                               (const int*)st.rows.p, (const int*)st.cols.p, st.k, t, b_kp.as<double>());
            PCR_HIP(ctx, hipGetLastError());
        }
        // the octave's cloud is the next one's input; the one before it goes back (the stream has passed every launch that read it: the
        // filter that made `down` waited behind them)
        if (cur.h) pcr_cloud_free(ctx, cur.release());
        cur.h = next.release();
        in = cur.h;
    }
    *n_out = total;
    if ((rc = sift_capacity(ctx, "pcr_sift", capacity, total))) return rc;
    if (total) {
        pcr_dev_block b_all(ctx);
        if ((rc = b_all.alloc(sizeof(double) * 5 * (size_t)total))) return rc;
        size_t at = 0;
        for (const kept& kv : octaves) {
            PCR_HIP(ctx, hipMemcpyAsync(b_all.as<double>() + 5 * at, kv.block->p, sizeof(double) * 5 * kv.k, hipMemcpyDeviceToDevice, ctx->stream));
            at += kv.k;
        }
        std::vector<double> all(5 * (size_t)total);
        if ((rc = pcr_d2h_staged(ctx, all.data(), b_all.p, sizeof(double) * 5 * (size_t)total))) return rc;
        at = 0;
        for (const kept& kv : octaves)
            for (unsigned int j = 0; j < kv.k; ++j, ++at) {
                memcpy(keypoints_out + 4 * at, all.data() + 5 * at, sizeof(double) * 4);
                if (octave_out) octave_out[at] = kv.octave;
                if (row_out) row_out[at] = (int32_t)all[5 * at + 4];
            }
    }
    return PCR_OK;
} PCR_CATCH(ctx)
