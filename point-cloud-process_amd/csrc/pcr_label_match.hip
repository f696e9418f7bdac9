// Label match: the per-label part of `process_sample` (Final_Project/scripts/extract.py:506-574) for all the KITTI 3-D labels of a
// frame in one launch over the grouped rows of a pcr_objects handle (include/pcr.h, "label match").
//   label_match_kernel     one workgroup of four waves per label.
//     phase A  the waves deal the objects among themselves (wave w: objects w, w + 4, ...).  An object whose stored box cannot meet
//              the label's sphere is not read (lm_box_outside); of the others a wave streams 64 rows at a time, one per lane (four such chunks in flight), and
//              counts the in-sphere rows and the in-sphere-and-in-box rows from ballot popcounts: exact integers, no atomics.  Each
//              wave leaves its k and its best (votes, object) in LDS; after ONE barrier every thread adds the four k and takes the
//              winner by (most votes, lowest id).
//     phase B  the winner's rows only.  Every wave walks all of them (position p in lane p % 64, chunks ascending: the order of the
//              object sum); wave a < 3 accumulates axis a, wave c % 4 stores the ballot of chunk c as one word of sel_bits.
// The label record and the calibration are wave-uniform: kernel arguments and scalar loads.  LDS holds the cross-wave combine only.
// The launch is latency-bound: at most L workgroups run, and each reads the grouped rows of the few objects near its label out of L2.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include "pcr_internal.h"
#include "pcr_kitti_dev.h"
#include "pcr_wave.h"

namespace {

constexpr int LM_WAVE = 64;
constexpr int LM_WAVES = 4;
constexpr int LM_BLOCK = LM_WAVE * LM_WAVES;
constexpr int LM_UNROLL = 4;                // chunks of 64 rows a wave has in flight
static_assert(LM_WAVES == 4, "phase B gives one axis to each of the first three waves and deals the ballot words by chunk & 3");

// one label as the kernel uses it; every derived value is exact (a halving) or written in the header (radius*radius)
struct lm_label {
    double v[3], rr;     // sphere centre, fl(radius * radius)
    double c[3];         // centre in the rectified camera frame
    double cs, sn;
    double hl, hh, hw;   // length/2, height/2, width/2
};

__device__ static inline lm_label lm_load(const double* __restrict__ rec) {
    lm_label q;
    q.v[0] = rec[0]; q.v[1] = rec[1]; q.v[2] = rec[2];
    q.rr = rec[3] * rec[3];
    q.c[0] = rec[4]; q.c[1] = rec[5]; q.c[2] = rec[6];
    q.cs = rec[7]; q.sn = rec[8];
    q.hl = rec[9] * 0.5; q.hh = rec[10] * 0.5; q.hw = rec[11] * 0.5;
    return q;
}

__device__ static inline bool lm_in_sphere(const lm_label& q, const pcr_pt& r) {
    const double dx = r.x - q.v[0], dy = r.y - q.v[1], dz = r.z - q.v[2];
    return (dx * dx + dy * dy) + dz * dz <= q.rr;
}

__device__ static inline bool lm_in_box(const kb_calib& k, const lm_label& q, const pcr_pt& r) {
    double X[3];
    kb_cam(k, r, X);
    const double e0 = X[0] - q.c[0], e1 = X[1] - q.c[1], e2 = X[2] - q.c[2];
    const double xo = q.cs * e0 - q.sn * e2, yo = e1 + q.hh, zo = q.sn * e0 + q.cs * e2;
    return -q.hl <= xo && xo <= q.hl && -q.hh <= yo && yo <= q.hh && -q.hw <= zo && zo <= q.hw;
}

// Whether NO row of an object with the axis-aligned box [bmin, bmax] (the exact minimum and maximum of its coordinates,
// pcr_objects_stats) can be in the sphere.  Per axis g = max(fl(bmin - v), fl(v - bmax), 0), then D = (gx*gx + gy*gy) + gz*gz in the
// order of in_sphere, and the object is skipped iff D > fl(r*r).
// Proof that a skipped object holds no in-sphere row.  Let x be a coordinate of one of its rows, bmin <= x <= bmax, and d = fl(x - v).
// Rounding to nearest is monotone (a <= b implies fl(a) <= fl(b)) and odd (fl(-a) = -fl(a)).  If bmin - v > 0 then x - v >= bmin - v, so
// d >= fl(bmin - v) > 0; if v - bmax > 0 then v - x >= v - bmax, so -d = fl(v - x) >= fl(v - bmax) > 0; at most one of the two holds;
// otherwise g = 0.  So |d| >= g >= 0 on every axis, hence d*d >= g*g as real numbers and fl(d*d) >= fl(g*g); a rounded sum of two
// numbers is monotone in each of them, so the row's (dx*dx + dy*dy) + dz*dz >= D step by step.  D > fl(r*r) therefore puts EVERY row
// of the object outside: the comparison is made on the very quantity in_sphere compares, not on a distance derived another way
// (fl(v - bmax) > r, say, does not exclude fl(d*d) == fl(r*r): that form would need a margin, this one needs none), so skipping
// changes neither k nor a vote nor any other bit.  A NaN coordinate was never a minimum or maximum and is in no sphere; an object
// without finite rows has bmin = +inf: D = +inf, skipped; a NaN D compares false: read.
__device__ static inline bool lm_box_outside(const lm_label& q, const double* __restrict__ st) {
    double g[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double below = st[3 + a] - q.v[a], above = q.v[a] - st[6 + a];
        g[a] = below > 0.0 ? below : (above > 0.0 ? above : 0.0);
    }
    return (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2] > q.rr;
}

// The rows first, first + 64, ... of an object of cnt > 0 rows, LM_UNROLL loads in flight before the first use: a wave walks an object
// alone, so the latency of one load per chunk is what it would otherwise wait for.  A row behind the end reads the object's last row
// instead (always a valid address); the caller masks it out.
__device__ static inline void lm_load_chunks(const pcr_pt* __restrict__ rows, long long cnt, long long first, pcr_pt (&r)[LM_UNROLL]) {
#pragma unroll
    for (int u = 0; u < LM_UNROLL; ++u) {
        const long long p = first + u * LM_WAVE;
        r[u] = rows[p < cnt ? p : cnt - 1];
    }
}

__global__ void __launch_bounds__(LM_BLOCK)
label_match_kernel(const pcr_pt* __restrict__ recs, const long long* __restrict__ off, const double* __restrict__ stats, int n_objects, kb_calib k,
                   const double* __restrict__ labels, double* __restrict__ result, unsigned long long* __restrict__ bits, long long words) {
    __shared__ long long s_k[LM_WAVES];
    __shared__ int s_votes[LM_WAVES], s_obj[LM_WAVES];
    const int lane = threadIdx.x & (LM_WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long l = blockIdx.x;
    const lm_label q = lm_load(labels + PCR_LABEL_DOUBLES * l);

    // phase A
    long long k_in = 0;
    int best_votes = 0, best_obj = -1;
    for (int o = wave; o < n_objects; o += LM_WAVES) {
        const long long base = off[o];
        const long long cnt = off[o + 1] - base;
        if (cnt <= 0 || lm_box_outside(q, stats + 9 * (long long)o)) continue;
        int votes = 0;
        for (long long j0 = 0; j0 < cnt; j0 += LM_UNROLL * LM_WAVE) {
            pcr_pt r[LM_UNROLL];
            lm_load_chunks(recs + base, cnt, j0 + lane, r);
#pragma unroll
            for (int u = 0; u < LM_UNROLL; ++u) {
                const bool in_s = j0 + u * LM_WAVE + lane < cnt && lm_in_sphere(q, r[u]);
                const bool in_b = in_s && lm_in_box(k, q, r[u]);
                k_in += __popcll(__ballot(in_s));
                votes += __popcll(__ballot(in_b));
            }
        }
        if (votes > best_votes) { best_votes = votes; best_obj = o; }   // (ascending o within a wave: the first maximum stays)
    }
    if (lane == 0) { s_k[wave] = k_in; s_votes[wave] = best_votes; s_obj[wave] = best_obj; }
    __syncthreads();
    long long k_all = 0;
    int win_votes = 0, win = -1;
#pragma unroll
    for (int w = 0; w < LM_WAVES; ++w) {
        k_all += s_k[w];
        const int v = s_votes[w], o = s_obj[w];
        if (v > win_votes || (v == win_votes && v > 0 && o < win)) { win_votes = v; win = o; }
    }

    // phase B
    double* const out = result + PCR_LABEL_RESULT_DOUBLES * l;
    unsigned long long* const my_bits = bits ? bits + l * words : nullptr;
    long long chunks = 0, n_sel = 0;
    if (win >= 0) {
        const long long base = off[win];
        const long long cnt = off[win + 1] - base;
        chunks = (cnt + LM_WAVE - 1) / LM_WAVE;
        double part = 0.0;
        for (long long c0 = 0; c0 < chunks; c0 += LM_UNROLL) {
            pcr_pt r[LM_UNROLL];
            lm_load_chunks(recs + base, cnt, c0 * LM_WAVE + lane, r);
#pragma unroll
            for (int u = 0; u < LM_UNROLL; ++u) {   // ascending chunks: the order of the lane partials
                const long long c = c0 + u;
                const bool sel = c * LM_WAVE + lane < cnt && lm_in_sphere(q, r[u]);
                const unsigned long long mask = __ballot(sel);   // (a chunk behind the last one: no lane is live, zero)
                n_sel += __popcll(mask);
                if (sel) part += wave == 0 ? r[u].x : (wave == 1 ? r[u].y : r[u].z);
                if (my_bits && c < chunks && c < words && (int)(c & (LM_WAVES - 1)) == wave && lane == 0) my_bits[c] = mask;
            }
        }
        const double total = wave_object_sum_f64(part);
        if (wave < 3 && lane == 0) out[4 + wave] = total / (double)n_sel;
    } else if (threadIdx.x < 3) {
        out[4 + threadIdx.x] = __longlong_as_double(0x7ff8000000000000ll);
    }
    if (my_bits)
        for (long long w = chunks + threadIdx.x; w < words; w += LM_BLOCK) my_bits[w] = 0ull;
    if (threadIdx.x == 0) {
        out[0] = (double)k_all;
        out[1] = (double)win;
        out[2] = (double)win_votes;
        out[3] = (double)n_sel;
        out[7] = 0.0;
    }
}

}  // namespace

extern "C" {

int pcr_objects_match_labels(pcr_ctx* ctx, const pcr_objects* objs, const pcr_kitti_calib* calib, const double* labels, int64_t L, double* result,
                             uint64_t* sel_bits, int64_t words) {
    if (!ctx || !objs || !calib || !result || L < 0 || (L > 0 && !labels)) return PCR_E_INVALID;
    kb_calib k;
    memcpy(k.T, calib->Tr_velo_to_cam, sizeof(k.T));
    memcpy(k.R0, calib->R0_rect, sizeof(k.R0));
    memcpy(k.P, calib->P2, sizeof(k.P));
    for (double v : k.T) if (!std::isfinite(v)) return PCR_E_INVALID;
    for (double v : k.R0) if (!std::isfinite(v)) return PCR_E_INVALID;
    for (double v : k.P) if (!std::isfinite(v)) return PCR_E_INVALID;
    for (int64_t l = 0; l < L; ++l) {
        const double* const rec = labels + PCR_LABEL_DOUBLES * l;
        for (int i = 0; i < 12; ++i) if (!std::isfinite(rec[i])) return PCR_E_INVALID;
        if (rec[3] < 0.0 || rec[9] < 0.0 || rec[10] < 0.0 || rec[11] < 0.0) return PCR_E_INVALID;
        for (int i = 12; i < PCR_LABEL_DOUBLES; ++i) if (!(rec[i] == 0.0)) return PCR_E_INVALID;
    }
    const int64_t n_objects = objs->n_objects;
    int64_t max_count = 0;
    for (int64_t o = 0; o < n_objects; ++o) max_count = std::max(max_count, objs->off[(size_t)o + 1] - objs->off[(size_t)o]);
    if (sel_bits && (words < 0 || words < (max_count + LM_WAVE - 1) / LM_WAVE)) return PCR_E_INVALID;
    if (L == 0) return PCR_OK;
    if (L > std::numeric_limits<int32_t>::max() || n_objects > std::numeric_limits<int32_t>::max()) return PCR_E_UNSUPPORTED;
    const size_t n_words = sel_bits ? (size_t)L * (size_t)words : 0;
    if (objs->m == 0) {   // no labelled rows: nothing to read, nothing to launch
        for (int64_t l = 0; l < L; ++l) {
            double* const out = result + PCR_LABEL_RESULT_DOUBLES * l;
            out[0] = 0.0; out[1] = -1.0; out[2] = 0.0; out[3] = 0.0;
            out[4] = out[5] = out[6] = std::numeric_limits<double>::quiet_NaN();
            out[7] = 0.0;
        }
        if (n_words) memset(sel_bits, 0, sizeof(uint64_t) * n_words);
        return PCR_OK;
    }
    hipSetDevice(ctx->device);
    pcr_dev_block b_labels(ctx), b_result(ctx), b_bits(ctx);
    int rc;
    if ((rc = b_labels.alloc(sizeof(double) * PCR_LABEL_DOUBLES * (size_t)L)) || (rc = b_result.alloc(sizeof(double) * PCR_LABEL_RESULT_DOUBLES * (size_t)L))) return rc;
    if (n_words && (rc = b_bits.alloc(sizeof(uint64_t) * n_words))) return rc;
    PCR_HIP(ctx, hipMemcpyAsync(b_labels.p, labels, sizeof(double) * PCR_LABEL_DOUBLES * (size_t)L, hipMemcpyHostToDevice, ctx->stream));
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "a ballot is one word of sel_bits");
    hipLaunchKernelGGL(label_match_kernel, dim3((unsigned int)L), dim3(LM_BLOCK), 0, ctx->stream, (const pcr_pt*)objs->recs, (const long long*)objs->d_off,
                       (const double*)objs->d_stats, (int)n_objects, k, b_labels.as<const double>(), b_result.as<double>(), b_bits.as<unsigned long long>(),
                       (long long)words);
    PCR_HIP(ctx, hipGetLastError());
    if (n_words) PCR_HIP(ctx, hipMemcpyAsync(sel_bits, b_bits.p, sizeof(uint64_t) * n_words, hipMemcpyDeviceToHost, ctx->stream));
    return pcr_d2h_small(ctx, result, b_result.p, sizeof(double) * PCR_LABEL_RESULT_DOUBLES * (size_t)L);   // (waits for the stream: `labels` is the caller's again)
}

}  // extern "C"
