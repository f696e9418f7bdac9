// SHOT352 at keypoint POSITIONS -- featureSHOT352 / featureSHOT352WithNormal of PCLKeypoints/src/keypoints.cpp, by the rules stated in
// include/pcr.h (PCL itself is not part of the build: parity with its binary32 output is unpinned).  The keypoints are coordinates
// searched against the cloud as search surface; the ball has no cap and is WALKED, never stored: one wave per keypoint over the grid
// with cell = radius (ball_grid), by the wave walk of pcr_ball_visit.h.  Two launches, nothing read back between them:
//   frames     shot_frame: walk 1, the seven weighted moments -- lane partials in walk order, combined by the xor butterfly
//              (wave_sum_all) --, every lane then solves the same 3x3 system (pcr::sym3_jacobi) and holds the same axes; walk 2, the
//              integer sign counts of the x and the z axis; s == 0: the TIE walks -- one counts the ball's d2 into 1 024 LDS bins,
//              which names the bins that hold the ranks K/2-2 .. K/2+2 and the number of neighbours below them; the next compacts
//              the neighbours OF THOSE BINS (d2, row, sign bits) into LDS 64 at a time, and each block of candidates walks the ball
//              once more, every lane counting the neighbours of those bins that precede its candidate in (d2, row) order (they are
//              handed round by readlane): the rank.  The five candidates of ranks K/2-2 .. K/2+2 vote.  Three walks for a usual
//              ball; O(c^2 / 64) comparisons a lane for c candidates, c = K only when every d2 falls into one bin.  No sort.
//   histogram  shot_hist_kernel: the frame is READ (the frames stage's, or the caller's frames_in: one code path, so frames_in =
//              an earlier frames_out reproduces the bytes); walk 3 compacts the in-ball positions into LDS and takes 64 neighbours
//              at a time, every lane busy: at most six (slot, value) pairs each, quantised to multiples of 2^-32 and added to a
//              352-bin LDS histogram with 64-bit INTEGER atomics -- the sums are exact, so their order is free.  No float atomics.
//              Norm: lane l adds the squares of its bins l, l + 64, ... in ascending order, the lanes' partials by the xor butterfly.
// pcr_shot_lrf is the frames launch alone.  Walk order = block cell 0..26, then stored order: a function of the surface in caller-row
// order, of the radius and of the keypoint's cell -- not of the other keypoints.
#include <cmath>
#include <cstring>
#include <string>
#include "pcr_ball_visit.h"
#include "pcr_linalg.h"

constexpr int SHOT_STAGE = 128;   // staged in-ball entries of the tie walk and of the histogram walk: < 64 left over + <= 64 of a trip
constexpr int SHOT_TIE_BINS = 1024;   // bins of d2 over [0, r^2] that narrow the tie walk down to the neighbours around the median
constexpr int SHOT_BINS = 352;
constexpr double SHOT_Q = 4294967296.0;   // 2^32
constexpr double SHOT_Q4 = 0.785398163397448309615660845819875721, SHOT_Q2 = 1.57079632679489661923132169163975144,
                 SHOT_Q34 = 2.35619449019234492884698253745962716, SHOT_Q78 = 2.74889357189106908365481296036956502;

__device__ static inline double dot3(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// v = p - x and its squared length (the ball predicate's left side: dist2's bits)
__device__ static inline double shot_rel(const pcr_pt& p, double x, double y, double z, double v[3]) {
    v[0] = p.x - x; v[1] = p.y - y; v[2] = p.z - z;
    return (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
}

// the sign that makes the component of largest magnitude positive (the first such of equal magnitudes)
__device__ static inline void shot_canonical(double a[3]) {
    const double m0 = fabs(a[0]), m1 = fabs(a[1]), m2 = fabs(a[2]);
    const double lead = (m0 >= m1 && m0 >= m2) ? a[0] : (m1 >= m2 ? a[1] : a[2]);
    if (lead < 0.0) { a[0] = -a[0]; a[1] = -a[1]; a[2] = -a[2]; }
}

// The local reference frame of the keypoint (x, y, z): F = rows x, y, z (the same bits in every lane), returns K = |B(x)|.
// t_d2 / t_id / t_fl: SHOT_STAGE entries of LDS each, t_hist: SHOT_TIE_BINS, t_sel: 3 -- used by the tie walk alone.  All 64 lanes
// must be active.
__device__ static inline int shot_frame(const pcr_grid_view& gv, double x, double y, double z, double r, double r2, unsigned int s, unsigned int e, int lane,
                                        double* t_d2, long long* t_id, unsigned int* t_fl, unsigned int* t_hist, int* t_sel, double F[9]) {
    // walk 1: moments
    double m[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int K = 0;
    auto moments = [&](unsigned int j, bool valid) {
        if (!valid) return;
        double v[3];
        const double d2 = shot_rel(gv.pts[j], x, y, z, v);
        if (!(d2 <= r2)) return;
        const double w = r - sqrt(d2);
        const double wx = w * v[0], wy = w * v[1], wz = w * v[2];
        m[0] += wx * v[0]; m[1] += wx * v[1]; m[2] += wx * v[2]; m[3] += wy * v[1]; m[4] += wy * v[2]; m[5] += wz * v[2]; m[6] += w;
        ++K;
    };
    wave_visit_runs(s, e, lane, moments);
#pragma unroll
    for (int k = 0; k < 7; ++k) m[k] = wave_sum_all(m[k]);
    K = wave_sum_all(K);
    if (K < 5 || !(m[6] > 0.0)) {
#pragma unroll
        for (int k = 0; k < 9; ++k) F[k] = NAN;
        return K;
    }
    double A[3][3], Q[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    A[0][0] = m[0] / m[6]; A[0][1] = A[1][0] = m[1] / m[6]; A[0][2] = A[2][0] = m[2] / m[6];
    A[1][1] = m[3] / m[6]; A[1][2] = A[2][1] = m[4] / m[6]; A[2][2] = m[5] / m[6];
    pcr::sym3_jacobi(A, Q);
    const double e0 = A[0][0], e1 = A[1][1], e2 = A[2][2];
    // (stable: of equal eigenvalues the first is the smallest, the last the largest)
    const int lo = (e1 < e0) ? ((e2 < e1) ? 2 : 1) : ((e2 < e0) ? 2 : 0);
    const int hi = (e1 >= e0) ? ((e2 >= e1) ? 2 : 1) : ((e2 >= e0) ? 2 : 0);
    double ax[3], az[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        ax[i] = hi == 0 ? Q[i][0] : (hi == 1 ? Q[i][1] : Q[i][2]);
        az[i] = lo == 0 ? Q[i][0] : (lo == 1 ? Q[i][1] : Q[i][2]);
    }
    const double nx = sqrt(dot3(ax, ax)), nz = sqrt(dot3(az, az));
#pragma unroll
    for (int i = 0; i < 3; ++i) { ax[i] /= nx; az[i] /= nz; }
    // the solver's sign is replaced by a rule (the component of largest magnitude is positive): with rows AT the keypoint both signs
    // of an axis can satisfy the sign rule below, and the frame must not depend on the solver
    shot_canonical(ax);
    shot_canonical(az);
    // walk 2: signs
    int px = 0, pz = 0;
    auto signs = [&](unsigned int j, bool valid) {
        if (!valid) return;
        double v[3];
        const double d2 = shot_rel(gv.pts[j], x, y, z, v);
        if (!(d2 <= r2)) return;
        px += dot3(v, ax) >= 0.0 ? 1 : 0;
        pz += dot3(v, az) >= 0.0 ? 1 : 0;
    };
    wave_visit_runs(s, e, lane, signs);
    px = wave_sum_all(px);
    pz = wave_sum_all(pz);
    const int sx = 2 * px - K, sz = 2 * pz - K;
    int mx = 0, mz = 0;   // of the five median neighbours, those strictly on the plus side
    if (sx == 0 || sz == 0) {   // (wave-uniform) the tie walk
        const int r_lo = K / 2 - 2, r_hi = K / 2 + 2;
        // First the ball's d2 are counted into SHOT_TIE_BINS bins (monotone in d2, so a smaller bin is a smaller d2): the bins that
        // hold the ranks r_lo and r_hi, and how many neighbours lie in the bins below.  Only neighbours of those bins are candidates,
        // and only they are compared with: a dozen of a ball of two thousand, unless the d2 crowd together (a sphere around x).
        const double scale = (double)SHOT_TIE_BINS / r2;
        auto bin_of = [&](double d2) { const int b = (int)(d2 * scale); return b < SHOT_TIE_BINS - 1 ? b : SHOT_TIE_BINS - 1; };
        for (int b = lane; b < SHOT_TIE_BINS; b += 64) t_hist[b] = 0u;
        __syncthreads();
        auto count = [&](unsigned int j, bool valid) {
            if (!valid) return;
            double v[3];
            const double d2 = shot_rel(gv.pts[j], x, y, z, v);
            if (d2 <= r2) atomicAdd(&t_hist[bin_of(d2)], 1u);
        };
        wave_visit_runs(s, e, lane, count);
        __syncthreads();
        constexpr int OWN = SHOT_TIE_BINS / 64;   // lane l owns the bins OWN l .. OWN l + OWN - 1
        unsigned int own = 0;
        for (int k = 0; k < OWN; ++k) own += t_hist[OWN * lane + k];
        unsigned int total;
        unsigned int run = wave_excl_scan_u32(own, lane, &total);   // the neighbours in the bins below this lane's
        for (int k = 0; k < OWN; ++k) {
            const unsigned int c = t_hist[OWN * lane + k];
            if (run <= (unsigned int)r_lo && (unsigned int)r_lo < run + c) { t_sel[0] = OWN * lane + k; t_sel[1] = (int)run; }
            if (run <= (unsigned int)r_hi && (unsigned int)r_hi < run + c) t_sel[2] = OWN * lane + k;
            run += c;
        }
        __syncthreads();
        const int bin_lo = t_sel[0], below = t_sel[1], bin_hi = t_sel[2];
        auto near_median = [&](double d2) { const int b = bin_of(d2); return d2 <= r2 && b >= bin_lo && b <= bin_hi; };
        int staged = 0;
        auto rank_block = [&](int base, int cnt) {
            const bool have = lane < cnt;
            const double cd2 = have ? t_d2[base + lane] : 0.0;
            const long long cid = have ? t_id[base + lane] : 0;
            const unsigned int fl = have ? t_fl[base + lane] : 0u;
            int rank = below;
            auto before = [&](unsigned int j, bool valid) {
                double d2 = 0.0;
                long long id = 0;
                bool in = false;
                if (valid) {
                    const pcr_pt p = gv.pts[j];
                    double v[3];
                    d2 = shot_rel(p, x, y, z, v);
                    id = p.id;
                    in = near_median(d2);
                }
                unsigned long long mask = __ballot(in);
                while (mask) {
                    const int l = __builtin_ctzll(mask);
                    mask &= mask - 1ull;
                    const double bd2 = readlane_f64(d2, l);
                    const long long bid = readlane_i64(id, l);
                    rank += (bd2 < cd2 || (bd2 == cd2 && bid < cid)) ? 1 : 0;
                }
            };
            wave_visit_runs(s, e, lane, before);
            const bool mid = have && rank >= r_lo && rank <= r_hi;
            mx += __popcll(__ballot(mid && (fl & 1u)));
            mz += __popcll(__ballot(mid && (fl & 2u)));
        };
        auto candidates = [&](unsigned int j, bool valid) {
            double d2 = 0.0;
            long long id = 0;
            unsigned int fl = 0;
            bool in = false;
            if (valid) {
                const pcr_pt p = gv.pts[j];
                double v[3];
                d2 = shot_rel(p, x, y, z, v);
                id = p.id;
                in = near_median(d2);
                fl = (dot3(v, ax) > 0.0 ? 1u : 0u) | (dot3(v, az) > 0.0 ? 2u : 0u);
            }
            int add;
            const int at = staged + wave_compact_slot(in, lane, &add);
            if (in) { t_d2[at] = d2; t_id[at] = id; t_fl[at] = fl; }
            staged += add;
            if (staged >= 64) {
                __syncthreads();
                rank_block(staged - 64, 64);
                staged -= 64;
                __syncthreads();
            }
        };
        wave_visit_runs(s, e, lane, candidates);
        __syncthreads();
        if (staged > 0) rank_block(0, staged);
        __syncthreads();
    }
    const bool flip_x = sx < 0 || (sx == 0 && mx < 3), flip_z = sz < 0 || (sz == 0 && mz < 3);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        if (flip_x) ax[i] = -ax[i];
        if (flip_z) az[i] = -az[i];
    }
    F[0] = ax[0]; F[1] = ax[1]; F[2] = ax[2];
    F[3] = az[1] * ax[2] - az[2] * ax[1];   // y = z cross x
    F[4] = az[2] * ax[0] - az[0] * ax[2];
    F[5] = az[0] * ax[1] - az[1] * ax[0];
    F[6] = az[0]; F[7] = az[1]; F[8] = az[2];
    return K;
}

__global__ void __launch_bounds__(64) shot_frame_kernel(pcr_grid_view gv, const double* __restrict__ kp /* (m,3) */, double r, double r2, double* __restrict__ frames /* (m,9) */,
                                                        int* __restrict__ counts /* (m) */) {
    __shared__ double t_d2[SHOT_STAGE];
    __shared__ long long t_id[SHOT_STAGE];
    __shared__ unsigned int t_fl[SHOT_STAGE];
    __shared__ unsigned int t_hist[SHOT_TIE_BINS];
    __shared__ int t_sel[3];
    const int lane = threadIdx.x;
    const long long i = blockIdx.x;
    const double x = kp[3 * i], y = kp[3 * i + 1], z = kp[3 * i + 2];
    unsigned int s, e;
    wave_block_runs(gv, x, y, z, lane, &s, &e);
    double F[9];
    const int K = shot_frame(gv, x, y, z, r, r2, s, e, lane, t_d2, t_id, t_fl, t_hist, t_sel, F);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) frames[9 * i + k] = F[k];
        counts[i] = K;
    }
}

// one neighbour's contributions to the integer histogram
__device__ static inline void shot_add(unsigned long long* h, int slot, double v) {
    atomicAdd(&h[slot], (unsigned long long)(long long)rint(v * SHOT_Q));
}
__device__ static inline double shot_tiny(double v) { return fabs(v) < 1e-30 ? 0.0 : v; }
__device__ static inline double shot_clamp(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ static inline void shot_neighbour(const pcr_pt& p, const double* __restrict__ normals, double x, double y, double z, double r, const double F[9],
                                             unsigned long long* h) {
    double v[3];
    const double d2 = shot_rel(p, x, y, z, v);
    const double n[3] = {normals[3 * p.id], normals[3 * p.id + 1], normals[3 * p.id + 2]};
    if (!finite3(n[0], n[1], n[2]) || d2 == 0.0) return;
    const double r4 = 0.25 * r, rh = 0.5 * r, r34 = 0.75 * r;
    const double c = shot_clamp(dot3(n, F + 6), -1.0, 1.0);
    const double b = ((1.0 + c) * 10) / 2;
    const double X = shot_tiny(dot3(v, F)), Y = shot_tiny(dot3(v, F + 3)), Z = shot_tiny(dot3(v, F + 6));
    const double d = sqrt(d2);
    const int bit4 = (Y > 0 || (Y == 0.0 && X < 0)) ? 1 : 0;
    const int bit3 = (X > 0 || (X == 0.0 && Y > 0)) ? !bit4 : bit4;
    int desc = ((bit4 << 3) + (bit3 << 2)) << 1;
    if (X * Y > 0 || X == 0.0) desc += (fabs(X) >= fabs(Y)) ? 0 : 4;
    else desc += (fabs(X) > fabs(Y)) ? 4 : 0;
    desc += (Z > 0) ? 1 : 0;
    desc += (d > rh) ? 2 : 0;
    const int sel = desc >> 2;
    int step = (int)floor(b + 0.5);
    step = step < 0 ? 0 : (step > 10 ? 10 : step);   // (b lies in 0..10: this only keeps a NaN from a wild normal inside the histogram)
    const double rho = b - step;
    const int vol = desc * 11;
    double W = 1.0 - fabs(rho);
    if (rho > 0) shot_add(h, vol + (step + 1) % 10, rho);
    else shot_add(h, vol + (step - 1 + 10) % 10, -rho);
    if (d > rh) {
        const double t = (d - r34) / rh;
        if (d > r34) W += 1 - t;
        else { W += 1 + t; shot_add(h, (desc - 2) * 11 + step, -t); }
    } else {
        const double t = (d - r4) / rh;
        if (d < r4) W += 1 + t;
        else { W += 1 - t; shot_add(h, (desc + 2) * 11 + step, t); }
    }
    const double theta = acos(shot_clamp(Z / d, -1.0, 1.0));
    if (Z <= 0) {
        const double u = (theta - SHOT_Q34) / SHOT_Q2;
        if (theta > SHOT_Q34) W += 1 - u;
        else { W += 1 + u; shot_add(h, (desc + 1) * 11 + step, -u); }
    } else {
        const double u = (theta - SHOT_Q4) / SHOT_Q2;
        if (theta < SHOT_Q4) W += 1 + u;
        else { W += 1 - u; shot_add(h, (desc - 1) * 11 + step, u); }
    }
    if (X != 0.0 || Y != 0.0) {
        const double a = shot_clamp((atan2(Y, X) - (-SHOT_Q78 + SHOT_Q4 * sel)) / SHOT_Q4, -0.5, 0.5);
        if (a > 0) { W += 1 - a; shot_add(h, ((desc + 4) % 32) * 11 + step, a); }
        else { W += 1 + a; shot_add(h, ((desc - 4 + 32) % 32) * 11 + step, -a); }
    }
    shot_add(h, vol + step, W);
}

__global__ void __launch_bounds__(64) shot_hist_kernel(pcr_grid_view gv, const double* __restrict__ kp /* (m,3) */, double r, double r2, const double* __restrict__ normals /* by row */,
                                                       const double* __restrict__ frames /* (m,9) */, double* __restrict__ out /* (m,352) */, int* __restrict__ counts /* (m) */) {
    __shared__ unsigned long long h[SHOT_BINS];
    __shared__ unsigned int s_pos[SHOT_STAGE];
    const int lane = threadIdx.x;
    const long long i = blockIdx.x;
    const double x = kp[3 * i], y = kp[3 * i + 1], z = kp[3 * i + 2];
    double F[9];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 9; ++k) { F[k] = frames[9 * i + k]; ok = ok && F[k] - F[k] == 0.0; }
    for (int b = lane; b < SHOT_BINS; b += 64) h[b] = 0ull;
    unsigned int s, e;
    wave_block_runs(gv, x, y, z, lane, &s, &e);
    int staged = 0, K = 0;   // (the same in every lane)
    __syncthreads();
    auto trip = [&](unsigned int j, bool valid) {
        const bool in = valid && dist2(x, y, z, gv.pts[j]) <= r2;
        int add;
        const int at = staged + wave_compact_slot(in, lane, &add);
        K += add;
        if (!ok) return;   // (wave-uniform: the ball is only counted)
        if (in) s_pos[at] = j;
        staged += add;
        if (staged >= 64) {
            __syncthreads();
            shot_neighbour(gv.pts[s_pos[staged - 64 + lane]], normals, x, y, z, r, F, h);
            staged -= 64;
            __syncthreads();
        }
    };
    wave_visit_runs(s, e, lane, trip);
    __syncthreads();
    if (lane < staged) shot_neighbour(gv.pts[s_pos[lane]], normals, x, y, z, r, F, h);
    __syncthreads();
    if (lane == 0) counts[i] = K;
    // h_b = integer 2^-32; the norm: this lane's bins in ascending order, then the xor butterfly
    double hb[6], sq = 0.0;
#pragma unroll
    for (int t = 0; t < 6; ++t) {
        const int b = lane + 64 * t;
        hb[t] = b < SHOT_BINS ? (double)(long long)h[b] * (1.0 / SHOT_Q) : 0.0;
        sq += hb[t] * hb[t];
    }
    const double norm = sqrt(wave_sum_all(sq));
#pragma unroll
    for (int t = 0; t < 6; ++t) {
        const int b = lane + 64 * t;
        if (b < SHOT_BINS) out[SHOT_BINS * i + b] = ok ? hb[t] / norm : NAN;
    }
}

// the arguments both entry points share, checked before anything is launched or allocated
static int shot_args(pcr_ctx* ctx, const pcr_cloud* surface, const double* keypoints, int64_t m, double radius) {
    if (!ctx || !surface || m < 0 || !(radius > 0) || !std::isfinite(radius)) return PCR_E_INVALID;
    if (m > 0 && !keypoints) return PCR_E_INVALID;
    if (m > 0x7fffffffLL) return PCR_E_INVALID;   // (one block per keypoint)
    return PCR_OK;
}

extern "C" int pcr_shot_lrf(pcr_ctx* ctx, const pcr_cloud* surface, const double* keypoints, int64_t m, double radius, double* frames_out, int32_t* counts_out) try {
    int rc = shot_args(ctx, surface, keypoints, m, radius);
    if (rc) return rc;
    if (m > 0 && !frames_out) return PCR_E_INVALID;
    if (surface->n <= 0) return PCR_E_EMPTY;
    if (m == 0) return PCR_OK;
    hipSetDevice(ctx->device);
    pcr_index_guard idx(ctx);
    if ((rc = ball_grid(ctx, surface, radius, "pcr_shot_lrf", idx))) return rc;
    pcr_dev_block b_kp(ctx), b_frames(ctx), b_counts(ctx);
    if ((rc = b_kp.alloc(sizeof(double) * 3 * m)) || (rc = b_frames.alloc(sizeof(double) * 9 * m)) || (rc = b_counts.alloc(sizeof(int) * m))) return rc;
    PCR_HIP(ctx, hipMemcpyAsync(b_kp.p, keypoints, sizeof(double) * 3 * m, hipMemcpyHostToDevice, ctx->stream));
    pcr_prof_mark(ctx, 0);
    hipLaunchKernelGGL(shot_frame_kernel, dim3((unsigned)m), dim3(64), 0, ctx->stream, idx->view, (const double*)b_kp.p, radius, radius * radius, b_frames.as<double>(),
                       b_counts.as<int>());
    for (int k = 1; k <= 4; ++k) pcr_prof_mark(ctx, k);   // (one stage: the profile's other three read 0)
    PCR_HIP(ctx, hipGetLastError());
    PCR_HIP(ctx, hipMemcpyAsync(frames_out, b_frames.p, sizeof(double) * 9 * m, hipMemcpyDeviceToHost, ctx->stream));
    if (counts_out) PCR_HIP(ctx, hipMemcpyAsync(counts_out, b_counts.p, sizeof(int) * m, hipMemcpyDeviceToHost, ctx->stream));
    PCR_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the call's one wait
    pcr_prof_finish(ctx);
    return PCR_OK;
} PCR_CATCH(ctx)

extern "C" int pcr_shot352(pcr_ctx* ctx, const pcr_cloud* surface, const double* normals, const double* keypoints, int64_t m, double radius, const double* frames_in,
                           double* features_out, double* frames_out, int32_t* counts_out) try {
    int rc = shot_args(ctx, surface, keypoints, m, radius);
    if (rc) return rc;
    if (!normals || (m > 0 && !features_out)) return PCR_E_INVALID;
    if (surface->n <= 0) return PCR_E_EMPTY;
    if (m == 0) return PCR_OK;
    hipSetDevice(ctx->device);
    const int64_t n = surface->n;
    pcr_index_guard idx(ctx);
    if ((rc = ball_grid(ctx, surface, radius, "pcr_shot352", idx))) return rc;
    pcr_dev_block b_nrm(ctx), b_kp(ctx), b_frames(ctx), b_counts(ctx), b_out(ctx);
    if ((rc = b_nrm.alloc(sizeof(double) * 3 * n)) || (rc = b_kp.alloc(sizeof(double) * 3 * m)) || (rc = b_frames.alloc(sizeof(double) * 9 * m)) ||
        (rc = b_counts.alloc(sizeof(int) * m)) || (rc = b_out.alloc(sizeof(double) * SHOT_BINS * m)))
        return rc;
    const double r2 = radius * radius;
    PCR_HIP(ctx, hipMemcpyAsync(b_nrm.p, normals, sizeof(double) * 3 * n, hipMemcpyHostToDevice, ctx->stream));
    PCR_HIP(ctx, hipMemcpyAsync(b_kp.p, keypoints, sizeof(double) * 3 * m, hipMemcpyHostToDevice, ctx->stream));
    if (frames_in) PCR_HIP(ctx, hipMemcpyAsync(b_frames.p, frames_in, sizeof(double) * 9 * m, hipMemcpyHostToDevice, ctx->stream));
    pcr_prof_mark(ctx, 0);
    if (!frames_in)
        hipLaunchKernelGGL(shot_frame_kernel, dim3((unsigned)m), dim3(64), 0, ctx->stream, idx->view, (const double*)b_kp.p, radius, r2, b_frames.as<double>(), b_counts.as<int>());
    pcr_prof_mark(ctx, 1);
    hipLaunchKernelGGL(shot_hist_kernel, dim3((unsigned)m), dim3(64), 0, ctx->stream, idx->view, (const double*)b_kp.p, radius, r2, (const double*)b_nrm.p,
                       (const double*)b_frames.p, b_out.as<double>(), b_counts.as<int>());
    for (int k = 2; k <= 4; ++k) pcr_prof_mark(ctx, k);   // (two stages: frames, histogram)
    PCR_HIP(ctx, hipGetLastError());
    PCR_HIP(ctx, hipMemcpyAsync(features_out, b_out.p, sizeof(double) * SHOT_BINS * m, hipMemcpyDeviceToHost, ctx->stream));
    if (frames_out) PCR_HIP(ctx, hipMemcpyAsync(frames_out, b_frames.p, sizeof(double) * 9 * m, hipMemcpyDeviceToHost, ctx->stream));
    if (counts_out) PCR_HIP(ctx, hipMemcpyAsync(counts_out, b_counts.p, sizeof(int) * m, hipMemcpyDeviceToHost, ctx->stream));
    PCR_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the call's one wait
    pcr_prof_finish(ctx);
    return PCR_OK;
} PCR_CATCH(ctx)
