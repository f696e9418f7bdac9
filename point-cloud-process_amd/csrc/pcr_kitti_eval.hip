// KITTI evaluation (include/pcr.h, "KITTI evaluation"): box overlaps, the greedy detection-to-label matching and the average precision,
// for all frames at once.  The header's comment is the definition of every rule; this file is its launch shape.
//   ke_overlap_kernel     one workgroup per frame: the frame's rows (12 doubles each: the fields the overlaps read, cos and sin of ry)
//                         are staged in LDS, a thread takes the pairs p, p + 256, ... of the frame's nd x ng block and writes the image,
//                         ground and 3-D overlap of each (pcr_kitti_eval_dev.h, shared with the host's pcr_kitti_box_overlap).  The
//                         column of a don't-care label holds the criterion-0 overlap the matching asks of it: such a label never
//                         takes part in the label loop, so its union overlap has no reader.
//   ke_first_kernel       mode 1.  One wave per frame stages the cleaning flags of the nine (class, difficulty) pairs and the scores
//                         in LDS; lanes 0..26 each run the greedy loop of one (class, metric, difficulty) and append the scores they
//                         emit to that combination's list through an integer slot counter (the lists are sorted next: their order is
//                         immaterial), tp and fn through integer atomics.
//   rocprim::segmented_radix_sort_keys_desc over the 27 lists, then
//   ke_threshold_kernel   one thread per combination walks the recall grid over its sorted list: the thresholds stay on the device.
//   ke_second_kernel      mode 2, the hot one.  A workgroup of 256 threads walks the frames f = block, block + grid, ...; per frame it
//                         stages the flags, the scores and -- if the frame has at most KE_LDS_PAIRS pairs -- the three overlap
//                         matrices in LDS (48 KiB of matrices + 5.5 KiB of rows: two workgroups per compute unit); a larger frame
//                         reads its overlaps from global memory.  Thread t owns the combinations (class, metric, difficulty, threshold)
//                         t, t + 256, ... of the 27 x 41, for every frame; the assigned set is four 64-bit words in registers, and so
//                         are its tp, fp, fn until the workgroup has seen its last frame; then one integer atomic each.
// Integer sums are exact in any order; there is no floating-point atomic, and no floating-point sum across threads at all.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>
#include <rocprim/rocprim.hpp>
#include "pcr_internal.h"
#include "pcr_kitti_eval_dev.h"

namespace {

constexpr int KE_MAX_DET = PCR_KITTI_EVAL_MAX_DET, KE_MAX_GT = PCR_KITTI_EVAL_MAX_GT, KE_S = PCR_KITTI_EVAL_SAMPLES;
constexpr int KE_ROW = 18;                 // a row on the device: the caller's 16 doubles, cos(ry), sin(ry)
constexpr int KE_COMBOS = 27;              // (class*3 + metric)*3 + difficulty
constexpr int KE_WORK = KE_COMBOS * KE_S;  // 1 107 greedy loops per frame in mode 2
constexpr int KE_BLOCK = 256;
constexpr int KE_SLOTS = (KE_WORK + KE_BLOCK - 1) / KE_BLOCK;
constexpr int KE_LDS_PAIRS = 2048;         // 3 matrices x 2048 pairs x 8 B = 48 KiB
constexpr int KE_BOX = 12;                 // doubles of a staged box
static_assert(KE_MAX_DET == 256, "the assigned set is four 64-bit words");
static_assert(sizeof(double) * (3 * KE_LDS_PAIRS + KE_MAX_DET) + 9 * (KE_MAX_DET + KE_MAX_GT) <= 64 * 1024, "static LDS of the mode-2 kernel");
static_assert(sizeof(double) * KE_BOX * (KE_MAX_DET + KE_MAX_GT) + KE_MAX_GT <= 64 * 1024, "static LDS of the overlap kernel");

struct ke_min_overlap { double v[3][3]; };   // [metric][class]
// (nine selects: indexing a kernel argument with computed m, c would put the table into scratch memory)
__device__ static inline double ke_min_overlap_of(const ke_min_overlap& mo, int m, int c) {
    double r = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) r = (m == i && c == j) ? mo.v[i][j] : r;
    return r;
}

// ------------------------------------------------------------------ cleaning
__device__ static inline double ke_min_height(int d) { return d == 0 ? 40.0 : 25.0; }
__device__ static inline double ke_max_occlusion(int d) { return (double)d; }
__device__ static inline double ke_max_truncation(int d) { return d == 0 ? 0.15 : (d == 1 ? 0.30 : 0.50); }

// 0 counted, 1 ignored, -1 absent, 2 don't care
__device__ static inline int ke_gt_flag(const double* r, int c, int d) {
    const double type = r[0];
    if (type == 5.0) return 2;
    if (type == (double)c) return (r[2] > ke_max_occlusion(d) || r[1] > ke_max_truncation(d) || r[7] - r[5] < ke_min_height(d)) ? 1 : 0;
    if ((c == 0 && type == 3.0) || (c == 1 && type == 4.0)) return 1;
    return -1;
}
__device__ static inline int ke_det_flag(const double* r, int c, int d) {
    if (r[0] != (double)c) return -1;
    return r[7] - r[5] < ke_min_height(d) ? 1 : 0;
}

// the flags of the nine (class, difficulty) pairs and the scores of one frame -> LDS, by all threads of the workgroup
template <int BLOCK>
__device__ static inline void ke_stage_rows(const double* __restrict__ det, int nd, const double* __restrict__ gt, int ng, signed char (*s_df)[KE_MAX_DET],
                                            signed char (*s_gf)[KE_MAX_GT], double* s_sc) {
    for (int i = threadIdx.x; i < nd; i += BLOCK) {
        const double* const r = det + (long long)KE_ROW * i;
        s_sc[i] = r[15];
#pragma unroll
        for (int cd = 0; cd < 9; ++cd) s_df[cd][i] = (signed char)ke_det_flag(r, cd / 3, cd % 3);
    }
    for (int i = threadIdx.x; i < ng; i += BLOCK) {
        const double* const r = gt + (long long)KE_ROW * i;
#pragma unroll
        for (int cd = 0; cd < 9; ++cd) s_gf[cd][i] = (signed char)ke_gt_flag(r, cd / 3, cd % 3);
    }
}

// ------------------------------------------------------------------ the greedy loop
struct ke_mask {
    unsigned long long w0, w1, w2, w3;
    __device__ bool get(int d) const {
        const int w = d >> 6;
        const unsigned long long word = w == 0 ? w0 : (w == 1 ? w1 : (w == 2 ? w2 : w3));
        return (word >> (d & 63)) & 1ull;
    }
    __device__ void set(int d) {
        const int w = d >> 6;
        const unsigned long long bit = 1ull << (d & 63);
        w0 |= w == 0 ? bit : 0ull;
        w1 |= w == 1 ? bit : 0ull;
        w2 |= w == 2 ? bit : 0ull;
        w3 |= w == 3 ? bit : 0ull;
    }
};

struct ke_counts { int tp, fp, fn; };

// ov: the frame's nd x ng block of the metric, detection-major; df / gf: the flags of the (class, difficulty); sc: the scores
template <bool FIRST, typename EMIT>
__device__ static inline ke_counts ke_greedy(int nd, int ng, const double* ov, const signed char* df, const signed char* gf, const double* sc, double min_ov, double t,
                                             EMIT emit) {
    int tp = 0, fp = 0, fn = 0;
    ke_mask assigned = {0ull, 0ull, 0ull, 0ull};
    for (int g = 0; g < ng; ++g) {
        const int gfl = gf[g];
        if (gfl != 0 && gfl != 1) continue;
        int cand = -1;
        bool cand_ignored = false;
        double best_o = 0.0, best_s = 0.0;
        for (int d = 0; d < nd; ++d) {
            const int dfl = df[d];
            if (dfl < 0 || assigned.get(d)) continue;
            const double s = sc[d];
            if (!FIRST && s < t) continue;
            const double o = ov[d * ng + g];
            if (!(o > min_ov)) continue;
            if (FIRST) {
                if (cand < 0 || s > best_s) { cand = d; best_s = s; cand_ignored = dfl == 1; }
            } else if (dfl == 0) {
                if (o > best_o || cand_ignored) { best_o = o; cand = d; cand_ignored = false; }
            } else if (cand < 0) {
                cand = d;
                cand_ignored = true;
            }
        }
        if (cand < 0) {
            fn += gfl == 0 ? 1 : 0;
        } else {
            assigned.set(cand);
            if (gfl == 0 && !cand_ignored) {
                tp += 1;
                if (FIRST) emit(sc[cand]);
            }
        }
    }
    if (FIRST) return ke_counts{tp, 0, fn};
    for (int d = 0; d < nd; ++d) fp += (df[d] == 0 && !assigned.get(d) && sc[d] >= t) ? 1 : 0;
    for (int g = 0; g < ng; ++g) {
        if (gf[g] != 2) continue;
        for (int d = 0; d < nd; ++d) {
            if (df[d] != 0 || assigned.get(d) || !(sc[d] >= t)) continue;
            if (ov[d * ng + g] > min_ov) { assigned.set(d); fp -= 1; }
        }
    }
    return ke_counts{tp, fp, fn};
}

// ------------------------------------------------------------------ kernels
__global__ void __launch_bounds__(KE_BLOCK)
ke_overlap_kernel(const double* __restrict__ det, const double* __restrict__ gt, const long long* __restrict__ det_first, const long long* __restrict__ gt_first,
                  const long long* __restrict__ pair_first, long long total, int criterion, int dontcare_first, double* __restrict__ ov) {
    __shared__ double s_det[KE_MAX_DET][KE_BOX];
    __shared__ double s_gt[KE_MAX_GT][KE_BOX];
    __shared__ unsigned char s_dc[KE_MAX_GT];
    const long long f = blockIdx.x;
    const long long d0 = det_first[f], g0 = gt_first[f];
    const int nd = (int)(det_first[f + 1] - d0), ng = (int)(gt_first[f + 1] - g0);
    if (nd <= 0 || ng <= 0 || nd > KE_MAX_DET || ng > KE_MAX_GT) return;   // (the host has refused a frame beyond the caps)
    for (int i = threadIdx.x; i < nd + ng; i += KE_BLOCK) {
        const bool is_det = i < nd;
        const double* const r = is_det ? det + KE_ROW * (d0 + i) : gt + KE_ROW * (g0 + (i - nd));
        double* const s = is_det ? s_det[i] : s_gt[i - nd];
#pragma unroll
        for (int k = 0; k < 10; ++k) s[k] = r[4 + k];
        s[10] = r[16];
        s[11] = r[17];
        if (!is_det) s_dc[i - nd] = r[0] == 5.0 ? 1 : 0;
    }
    __syncthreads();
    const long long base = pair_first[f];
    const int pairs = nd * ng;
    for (int p = threadIdx.x; p < pairs; p += KE_BLOCK) {
        const int d = p / ng, g = p - d * ng;
        ke_box a, b;
        const double* const sa = s_det[d];
        const double* const sb = s_gt[g];
        a.left = sa[0]; a.top = sa[1]; a.right = sa[2]; a.bottom = sa[3]; a.h = sa[4]; a.w = sa[5]; a.l = sa[6]; a.cx = sa[7]; a.cy = sa[8]; a.cz = sa[9];
        a.cs = sa[10]; a.sn = sa[11];
        b.left = sb[0]; b.top = sb[1]; b.right = sb[2]; b.bottom = sb[3]; b.h = sb[4]; b.w = sb[5]; b.l = sb[6]; b.cx = sb[7]; b.cy = sb[8]; b.cz = sb[9];
        b.cs = sb[10]; b.sn = sb[11];
        double out[3];
        ke_overlaps(a, b, (dontcare_first && s_dc[g]) ? 0 : criterion, out);
        ov[base + p] = out[0];
        ov[total + base + p] = out[1];
        ov[2 * total + base + p] = out[2];
    }
}

constexpr int KE_FIRST_BLOCK = 64;

// n_scores[27]: slot counters; counts[27][3]: tp, fn, n_gt (the labels with flag 0)
__global__ void __launch_bounds__(KE_FIRST_BLOCK)
ke_first_kernel(const double* __restrict__ det, const double* __restrict__ gt, const long long* __restrict__ det_first, const long long* __restrict__ gt_first,
                const long long* __restrict__ pair_first, long long total, const double* __restrict__ ov, ke_min_overlap mo, const unsigned int* __restrict__ list_begin,
                const unsigned int* __restrict__ list_cap, double* __restrict__ lists, unsigned int* __restrict__ n_scores, unsigned long long* __restrict__ counts) {
    __shared__ signed char s_df[9][KE_MAX_DET];
    __shared__ signed char s_gf[9][KE_MAX_GT];
    __shared__ double s_sc[KE_MAX_DET];
    const long long f = blockIdx.x;
    const long long d0 = det_first[f], g0 = gt_first[f];
    const int nd = (int)(det_first[f + 1] - d0), ng = (int)(gt_first[f + 1] - g0);
    if (ng <= 0 || nd < 0 || nd > KE_MAX_DET || ng > KE_MAX_GT) return;
    ke_stage_rows<KE_FIRST_BLOCK>(det + KE_ROW * d0, nd, gt + KE_ROW * g0, ng, s_df, s_gf, s_sc);
    __syncthreads();
    const int cmd = threadIdx.x;
    if (cmd >= KE_COMBOS) return;
    const int c = cmd / 9, m = (cmd / 3) % 3, dif = cmd % 3;
    const unsigned int begin = list_begin[cmd], cap = list_cap[cmd];
    const ke_counts n = ke_greedy<true>(nd, ng, ov + m * total + pair_first[f], s_df[c * 3 + dif], s_gf[c * 3 + dif], s_sc, ke_min_overlap_of(mo, m, c), 0.0, [&](double score) {
        const unsigned int slot = atomicAdd(&n_scores[cmd], 1u);
        if (slot < cap) lists[begin + slot] = score;   // (a list holds one slot per label of the class: never more are emitted)
    });
    int n_gt = 0;
    for (int g = 0; g < ng; ++g) n_gt += s_gf[c * 3 + dif][g] == 0 ? 1 : 0;
    if (n.tp) atomicAdd(&counts[3 * cmd], (unsigned long long)n.tp);
    if (n.fn) atomicAdd(&counts[3 * cmd + 1], (unsigned long long)n.fn);
    if (n_gt) atomicAdd(&counts[3 * cmd + 2], (unsigned long long)n_gt);
}

__global__ void ke_list_ends_kernel(const unsigned int* __restrict__ list_begin, const unsigned int* __restrict__ list_cap, const unsigned int* __restrict__ n_scores,
                                    unsigned int* __restrict__ list_end) {
    const int cmd = threadIdx.x;
    if (cmd < KE_COMBOS) list_end[cmd] = list_begin[cmd] + (n_scores[cmd] < list_cap[cmd] ? n_scores[cmd] : list_cap[cmd]);
}

__global__ void ke_threshold_kernel(const double* __restrict__ sorted, const unsigned int* __restrict__ list_begin, const unsigned int* __restrict__ list_end,
                                    const unsigned long long* __restrict__ counts, double* __restrict__ thr, int* __restrict__ n_thr) {
    const int cmd = threadIdx.x;
    if (cmd >= KE_COMBOS) return;
    const double* const v = sorted + list_begin[cmd];
    const long long len = (long long)list_end[cmd] - (long long)list_begin[cmd];
    const double n_gt = (double)counts[3 * cmd + 2];
    double current = 0.0;
    int n = 0;
    for (long long i = 0; i < len && n < KE_S; ++i) {
        const double l = (double)(i + 1) / n_gt;
        const double r = i < len - 1 ? (double)(i + 2) / n_gt : l;
        if ((r - current) < (current - l) && i < len - 1) continue;
        thr[cmd * KE_S + n++] = v[i];
        current += 1.0 / 40.0;
    }
    for (int k = n; k < KE_S; ++k) thr[cmd * KE_S + k] = 0.0;
    n_thr[cmd] = n;
}

// counts[27][41][3]: tp, fp, fn
__global__ void __launch_bounds__(KE_BLOCK)
ke_second_kernel(const double* __restrict__ det, const double* __restrict__ gt, const long long* __restrict__ det_first, const long long* __restrict__ gt_first,
                 const long long* __restrict__ pair_first, long long total, long long F, const double* __restrict__ ov, ke_min_overlap mo, const double* __restrict__ thr,
                 const int* __restrict__ n_thr, unsigned long long* __restrict__ counts) {
    __shared__ double s_ov[3 * KE_LDS_PAIRS];
    __shared__ double s_sc[KE_MAX_DET];
    __shared__ signed char s_df[9][KE_MAX_DET];
    __shared__ signed char s_gf[9][KE_MAX_GT];
    int tp[KE_SLOTS], fp[KE_SLOTS], fn[KE_SLOTS];
#pragma unroll
    for (int u = 0; u < KE_SLOTS; ++u) tp[u] = fp[u] = fn[u] = 0;
    for (long long f = blockIdx.x; f < F; f += gridDim.x) {
        const long long d0 = det_first[f], g0 = gt_first[f];
        const int nd = (int)(det_first[f + 1] - d0), ng = (int)(gt_first[f + 1] - g0);
        if (nd < 0 || ng < 0 || nd > KE_MAX_DET || ng > KE_MAX_GT) continue;   // (uniform; the host has refused a frame beyond the caps)
        const int pairs = nd * ng;
        const bool in_lds = pairs <= KE_LDS_PAIRS;
        const long long base = pair_first[f];
        __syncthreads();   // the readers of the frame before are done
        ke_stage_rows<KE_BLOCK>(det + KE_ROW * d0, nd, gt + KE_ROW * g0, ng, s_df, s_gf, s_sc);
        if (in_lds)
            for (int i = threadIdx.x; i < 3 * pairs; i += KE_BLOCK) {
                const int m = i / pairs;
                s_ov[i] = ov[m * total + base + (i - m * pairs)];
            }
        __syncthreads();
        for (int slot = 0; slot < KE_SLOTS; ++slot) {
            const int j = threadIdx.x + slot * KE_BLOCK;
            if (j >= KE_WORK) break;
            const int cmd = j / KE_S, k = j - cmd * KE_S;
            if (k >= n_thr[cmd]) continue;
            const int c = cmd / 9, m = (cmd / 3) % 3, dif = cmd % 3;
            const double t = thr[j], min_ov = ke_min_overlap_of(mo, m, c);
            const ke_counts n = in_lds ? ke_greedy<false>(nd, ng, s_ov + m * pairs, s_df[c * 3 + dif], s_gf[c * 3 + dif], s_sc, min_ov, t, [](double) {})
                                       : ke_greedy<false>(nd, ng, ov + m * total + base, s_df[c * 3 + dif], s_gf[c * 3 + dif], s_sc, min_ov, t, [](double) {});
#pragma unroll
            for (int u = 0; u < KE_SLOTS; ++u) {
                tp[u] += u == slot ? n.tp : 0;
                fp[u] += u == slot ? n.fp : 0;
                fn[u] += u == slot ? n.fn : 0;
            }
        }
    }
#pragma unroll
    for (int u = 0; u < KE_SLOTS; ++u) {
        const int j = threadIdx.x + u * KE_BLOCK;
        if (j >= KE_WORK) continue;
        if (tp[u]) atomicAdd(&counts[3 * j], (unsigned long long)tp[u]);
        if (fp[u]) atomicAdd(&counts[3 * j + 1], (unsigned long long)fp[u]);
        if (fn[u]) atomicAdd(&counts[3 * j + 2], (unsigned long long)fn[u]);
    }
}

// ------------------------------------------------------------------ host
struct ke_frames {
    pcr_dev_block det, gt, det_first, gt_first, pair_first, ov;
    int64_t F = 0, D = 0, G = 0, total = 0;
    int64_t class_labels[3] = {0, 0, 0};
    std::vector<long long> h_pair_first;
    explicit ke_frames(pcr_ctx* c) : det(c), gt(c), det_first(c), gt_first(c), pair_first(c), ov(c) {}
};

static int ke_upload(pcr_ctx* ctx, pcr_dev_block& blk, const void* src, size_t bytes) {
    int rc;
    if ((rc = blk.alloc(bytes ? bytes : 8))) return rc;
    if (bytes) PCR_HIP(ctx, hipMemcpyAsync(blk.p, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    return PCR_OK;
}

static void ke_rows18(const double* rows, int64_t n, std::vector<double>& out) {
    out.resize((size_t)KE_ROW * (size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const double* const r = rows + PCR_KITTI_ROW_DOUBLES * i;
        double* const o = out.data() + (size_t)KE_ROW * (size_t)i;
        memcpy(o, r, sizeof(double) * PCR_KITTI_ROW_DOUBLES);
        o[16] = std::cos(r[14]);
        o[17] = std::sin(r[14]);
    }
}

// validate, then upload; nothing is launched and no output written before every check has passed
static int ke_prepare(pcr_ctx* ctx, const double* det, const int64_t* det_first, const double* gt, const int64_t* gt_first, int64_t F, ke_frames& fr) {
    if (!ctx || F < 0 || !det_first || !gt_first || det_first[0] != 0 || gt_first[0] != 0) return PCR_E_INVALID;
    for (int64_t f = 0; f < F; ++f)
        if (det_first[f + 1] < det_first[f] || gt_first[f + 1] < gt_first[f]) return PCR_E_INVALID;
    fr.F = F; fr.D = det_first[F]; fr.G = gt_first[F];
    if ((fr.D > 0 && !det) || (fr.G > 0 && !gt)) return PCR_E_INVALID;
    if (F > std::numeric_limits<int32_t>::max()) return PCR_E_UNSUPPORTED;
    fr.h_pair_first.assign((size_t)F + 1, 0);
    for (int64_t f = 0; f < F; ++f) {
        const int64_t nd = det_first[f + 1] - det_first[f], ng = gt_first[f + 1] - gt_first[f];
        if (nd > KE_MAX_DET || ng > KE_MAX_GT) return PCR_E_UNSUPPORTED;
        fr.h_pair_first[(size_t)f + 1] = fr.h_pair_first[(size_t)f] + nd * ng;
    }
    fr.total = fr.h_pair_first[(size_t)F];
    for (int64_t i = 0; i < fr.G; ++i) {
        const double type = gt[PCR_KITTI_ROW_DOUBLES * i];
        for (int c = 0; c < 3; ++c) fr.class_labels[c] += type == (double)c ? 1 : 0;
    }
    if (9 * fr.G > (int64_t)std::numeric_limits<uint32_t>::max()) return PCR_E_UNSUPPORTED;   // (the segmented sort indexes with 32 bits)
    hipSetDevice(ctx->device);
    std::vector<double> rows;
    int rc;
    ke_rows18(det, fr.D, rows);
    if ((rc = ke_upload(ctx, fr.det, rows.data(), sizeof(double) * rows.size()))) return rc;
    PCR_HIP(ctx, pcr_sync(ctx->stream));   // (`rows` is written again below)
    ke_rows18(gt, fr.G, rows);
    if ((rc = ke_upload(ctx, fr.gt, rows.data(), sizeof(double) * rows.size()))) return rc;
    static_assert(sizeof(long long) == sizeof(int64_t), "the first arrays go up as they are");
    if ((rc = ke_upload(ctx, fr.det_first, det_first, sizeof(int64_t) * ((size_t)F + 1)))) return rc;
    if ((rc = ke_upload(ctx, fr.gt_first, gt_first, sizeof(int64_t) * ((size_t)F + 1)))) return rc;
    if ((rc = ke_upload(ctx, fr.pair_first, fr.h_pair_first.data(), sizeof(long long) * ((size_t)F + 1)))) return rc;
    if ((rc = fr.ov.alloc(sizeof(double) * 3 * (size_t)(fr.total ? fr.total : 1)))) return rc;
    PCR_HIP(ctx, pcr_sync(ctx->stream));   // (`rows` leaves scope)
    return PCR_OK;
}

static int ke_run_overlaps(pcr_ctx* ctx, ke_frames& fr, int criterion, int dontcare_first) {
    if (fr.F == 0 || fr.total == 0) return PCR_OK;
    hipLaunchKernelGGL(ke_overlap_kernel, dim3((unsigned int)fr.F), dim3(KE_BLOCK), 0, ctx->stream, fr.det.as<const double>(), fr.gt.as<const double>(),
                       fr.det_first.as<const long long>(), fr.gt_first.as<const long long>(), fr.pair_first.as<const long long>(), (long long)fr.total, criterion,
                       dontcare_first, fr.ov.as<double>());
    PCR_HIP(ctx, hipGetLastError());
    return PCR_OK;
}

// mode 1 for all 27 combinations: the sorted lists, their ends and the (tp, fn, n_gt) sums stay on the device
struct ke_first {
    pcr_dev_block lists, sorted, words, counts, temp;   // words: begin[27], cap[27], end[27], n_scores[27]
    unsigned int begin[KE_COMBOS + 1];
    explicit ke_first(pcr_ctx* c) : lists(c), sorted(c), words(c), counts(c), temp(c) {}
    const unsigned int* d_begin() const { return words.as<unsigned int>(); }
    const unsigned int* d_cap() const { return words.as<unsigned int>() + KE_COMBOS; }
    unsigned int* d_end() const { return words.as<unsigned int>() + 2 * KE_COMBOS; }
    unsigned int* d_n() const { return words.as<unsigned int>() + 3 * KE_COMBOS; }
};

static ke_min_overlap ke_table(const pcr_kitti_eval_params* params) {
    ke_min_overlap mo;
    memcpy(mo.v, params->min_overlap, sizeof(mo.v));
    return mo;
}

static bool ke_params_ok(const pcr_kitti_eval_params* params) {
    if (!params) return false;
    for (int m = 0; m < 3; ++m)
        for (int c = 0; c < 3; ++c)
            if (!(std::isfinite(params->min_overlap[m][c]) && params->min_overlap[m][c] >= 0.0)) return false;
    return true;
}

static int ke_run_first(pcr_ctx* ctx, ke_frames& fr, const ke_min_overlap& mo, ke_first& fi) {
    unsigned int h_words[4 * KE_COMBOS] = {0};
    fi.begin[0] = 0;
    for (int cmd = 0; cmd < KE_COMBOS; ++cmd) {
        h_words[cmd] = fi.begin[cmd];
        h_words[KE_COMBOS + cmd] = (unsigned int)fr.class_labels[cmd / 9];
        h_words[2 * KE_COMBOS + cmd] = fi.begin[cmd];
        fi.begin[cmd + 1] = fi.begin[cmd] + (unsigned int)fr.class_labels[cmd / 9];
    }
    const size_t cap = fi.begin[KE_COMBOS];
    int rc;
    if ((rc = fi.lists.alloc(sizeof(double) * (cap ? cap : 1))) || (rc = fi.sorted.alloc(sizeof(double) * (cap ? cap : 1))) || (rc = fi.words.alloc(sizeof(h_words))) ||
        (rc = fi.counts.alloc(sizeof(unsigned long long) * 3 * KE_COMBOS)))
        return rc;
    PCR_HIP(ctx, hipMemcpyAsync(fi.words.p, h_words, sizeof(h_words), hipMemcpyHostToDevice, ctx->stream));
    PCR_HIP(ctx, pcr_sync(ctx->stream));   // (h_words is this frame's)
    PCR_HIP(ctx, hipMemsetAsync(fi.counts.p, 0, sizeof(unsigned long long) * 3 * KE_COMBOS, ctx->stream));
    if (fr.F == 0 || cap == 0) return PCR_OK;
    hipLaunchKernelGGL(ke_first_kernel, dim3((unsigned int)fr.F), dim3(KE_FIRST_BLOCK), 0, ctx->stream, fr.det.as<const double>(), fr.gt.as<const double>(),
                       fr.det_first.as<const long long>(), fr.gt_first.as<const long long>(), fr.pair_first.as<const long long>(), (long long)fr.total,
                       fr.ov.as<const double>(), mo, fi.d_begin(), fi.d_cap(), fi.lists.as<double>(), fi.d_n(), fi.counts.as<unsigned long long>());
    PCR_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(ke_list_ends_kernel, dim3(1), dim3(64), 0, ctx->stream, fi.d_begin(), fi.d_cap(), (const unsigned int*)fi.d_n(), fi.d_end());
    PCR_HIP(ctx, hipGetLastError());
    size_t temp_bytes = 0;
    PCR_HIP(ctx, rocprim::segmented_radix_sort_keys_desc(nullptr, temp_bytes, fi.lists.as<double>(), fi.sorted.as<double>(), (unsigned int)cap, (unsigned int)KE_COMBOS,
                                                         fi.d_begin(), (const unsigned int*)fi.d_end(), 0u, 64u, ctx->stream));
    if ((rc = fi.temp.alloc(temp_bytes ? temp_bytes : 8))) return rc;
    PCR_HIP(ctx, rocprim::segmented_radix_sort_keys_desc(fi.temp.p, temp_bytes, fi.lists.as<double>(), fi.sorted.as<double>(), (unsigned int)cap, (unsigned int)KE_COMBOS,
                                                         fi.d_begin(), (const unsigned int*)fi.d_end(), 0u, 64u, ctx->stream));
    return PCR_OK;
}

// mode 2 with the thresholds at d_thr[27][41], d_n_thr[27] -> d_counts[27][41][3], zeroed here
static int ke_run_second(pcr_ctx* ctx, ke_frames& fr, const ke_min_overlap& mo, const double* d_thr, const int* d_n_thr, unsigned long long* d_counts) {
    PCR_HIP(ctx, hipMemsetAsync(d_counts, 0, sizeof(unsigned long long) * 3 * KE_WORK, ctx->stream));
    if (fr.F == 0) return PCR_OK;
    const long long grid = std::min<long long>(fr.F, 2ll * (ctx->cu_count > 0 ? ctx->cu_count : 256));
    hipLaunchKernelGGL(ke_second_kernel, dim3((unsigned int)grid), dim3(KE_BLOCK), 0, ctx->stream, fr.det.as<const double>(), fr.gt.as<const double>(),
                       fr.det_first.as<const long long>(), fr.gt_first.as<const long long>(), fr.pair_first.as<const long long>(), (long long)fr.total, (long long)fr.F,
                       fr.ov.as<const double>(), mo, d_thr, d_n_thr, d_counts);
    PCR_HIP(ctx, hipGetLastError());
    return PCR_OK;
}

static int ke_download(pcr_ctx* ctx, void* dst, const void* src, size_t bytes) {
    if (!bytes) return PCR_OK;
    PCR_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    PCR_HIP(ctx, pcr_sync(ctx->stream));
    return PCR_OK;
}

struct ke_events {   // the stage stopwatch of pcr_kitti_eval, only when the caller asks for it
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    bool on = false;
    ~ke_events() { for (hipEvent_t e : ev) if (e) hipEventDestroy(e); }
};

}  // namespace

extern "C" {

void pcr_kitti_eval_default_params(pcr_kitti_eval_params* params) {
    if (!params) return;
    memset(params, 0, sizeof(*params));
    for (int m = 0; m < 3; ++m) {
        params->min_overlap[m][0] = 0.7;
        params->min_overlap[m][1] = 0.5;
        params->min_overlap[m][2] = 0.5;
    }
}

int pcr_kitti_box_overlap(const double a[16], const double b[16], int metric, int criterion, double* out) {
    if (!a || !b || !out || metric < 0 || metric > 2 || criterion < -1 || criterion > 1) return PCR_E_INVALID;
    double o[3];
    ke_overlaps(ke_box_from_row(a, std::cos(a[14]), std::sin(a[14])), ke_box_from_row(b, std::cos(b[14]), std::sin(b[14])), criterion, o);
    *out = o[metric];
    return PCR_OK;
}

int pcr_kitti_eval_overlaps(pcr_ctx* ctx, const double* det, const int64_t* det_first, const double* gt, const int64_t* gt_first, int64_t F, int criterion,
                            double* image_out, double* ground_out, double* volume_out, int64_t* pair_first_out) try {
    if (!ctx || criterion < -1 || criterion > 1) return PCR_E_INVALID;
    ke_frames fr(ctx);
    int rc;
    if ((rc = ke_prepare(ctx, det, det_first, gt, gt_first, F, fr)) || (rc = ke_run_overlaps(ctx, fr, criterion, 0))) return rc;
    double* const outs[3] = {image_out, ground_out, volume_out};
    for (int m = 0; m < 3; ++m)
        if (outs[m] && fr.total && (rc = pcr_d2h_staged(ctx, outs[m], fr.ov.as<double>() + (size_t)m * (size_t)fr.total, sizeof(double) * (size_t)fr.total))) return rc;
    PCR_HIP(ctx, pcr_sync(ctx->stream));
    if (pair_first_out)
        for (int64_t f = 0; f <= F; ++f) pair_first_out[f] = fr.h_pair_first[(size_t)f];
    return PCR_OK;
} PCR_CATCH(ctx)

int pcr_kitti_eval_match(pcr_ctx* ctx, const double* det, const int64_t* det_first, const double* gt, const int64_t* gt_first, int64_t F,
                         const pcr_kitti_eval_params* params, int cls, int difficulty, int metric, const double* thresholds, int n_thresholds, int mode,
                         int64_t* tp_out, int64_t* fp_out, int64_t* fn_out, double* scores_out, int64_t* n_scores_out) try {
    if (!ctx || !ke_params_ok(params) || cls < 0 || cls > 2 || difficulty < 0 || difficulty > 2 || metric < 0 || metric > 2 || (mode != 1 && mode != 2))
        return PCR_E_INVALID;
    if (mode == 2 && (n_thresholds < 0 || n_thresholds > KE_S || (n_thresholds > 0 && !thresholds) || !tp_out || !fp_out || !fn_out)) return PCR_E_INVALID;
    if (mode == 1 && (!scores_out || !n_scores_out)) return PCR_E_INVALID;
    ke_frames fr(ctx);
    const ke_min_overlap mo = ke_table(params);
    const int cmd = (cls * 3 + metric) * 3 + difficulty;
    int rc;
    if ((rc = ke_prepare(ctx, det, det_first, gt, gt_first, F, fr)) || (rc = ke_run_overlaps(ctx, fr, -1, 1))) return rc;
    if (mode == 1) {
        ke_first fi(ctx);
        if ((rc = ke_run_first(ctx, fr, mo, fi))) return rc;
        unsigned int h_words[4 * KE_COMBOS];
        unsigned long long h_counts[3 * KE_COMBOS];
        if ((rc = ke_download(ctx, h_words, fi.words.p, sizeof(h_words))) || (rc = ke_download(ctx, h_counts, fi.counts.p, sizeof(h_counts)))) return rc;
        const unsigned int n = h_words[2 * KE_COMBOS + cmd] - h_words[cmd];
        if ((rc = ke_download(ctx, scores_out, fi.sorted.as<double>() + fi.begin[cmd], sizeof(double) * n))) return rc;
        *n_scores_out = n;
        if (tp_out) tp_out[0] = (int64_t)h_counts[3 * cmd];
        if (fn_out) fn_out[0] = (int64_t)h_counts[3 * cmd + 1];
        if (fp_out) fp_out[0] = (int64_t)h_counts[3 * cmd + 2];   // (mode 1 has no false positives: the slot carries n_gt)
        return PCR_OK;
    }
    pcr_dev_block b_thr(ctx), b_n(ctx), b_counts(ctx);
    std::vector<double> h_thr((size_t)KE_WORK, 0.0);
    int h_n[KE_COMBOS] = {0};
    for (int k = 0; k < n_thresholds; ++k) h_thr[(size_t)cmd * KE_S + k] = thresholds[k];
    h_n[cmd] = n_thresholds;
    if ((rc = ke_upload(ctx, b_thr, h_thr.data(), sizeof(double) * KE_WORK)) || (rc = ke_upload(ctx, b_n, h_n, sizeof(h_n))) ||
        (rc = b_counts.alloc(sizeof(unsigned long long) * 3 * KE_WORK)))
        return rc;
    PCR_HIP(ctx, pcr_sync(ctx->stream));
    if ((rc = ke_run_second(ctx, fr, mo, b_thr.as<const double>(), b_n.as<const int>(), b_counts.as<unsigned long long>()))) return rc;
    std::vector<unsigned long long> h_counts((size_t)3 * KE_WORK);
    if ((rc = ke_download(ctx, h_counts.data(), b_counts.p, sizeof(unsigned long long) * h_counts.size()))) return rc;
    for (int k = 0; k < n_thresholds; ++k) {
        const size_t j = (size_t)cmd * KE_S + k;
        tp_out[k] = (int64_t)h_counts[3 * j];
        fp_out[k] = (int64_t)h_counts[3 * j + 1];
        fn_out[k] = (int64_t)h_counts[3 * j + 2];
    }
    return PCR_OK;
} PCR_CATCH(ctx)

int pcr_kitti_eval(pcr_ctx* ctx, const double* det, const int64_t* det_first, const double* gt, const int64_t* gt_first, int64_t F,
                   const pcr_kitti_eval_params* params, pcr_kitti_eval_result* result, double* stage_ms) try {
    if (!ctx || !result || !ke_params_ok(params)) return PCR_E_INVALID;
    ke_frames fr(ctx);
    ke_first fi(ctx);
    ke_events ev;
    const ke_min_overlap mo = ke_table(params);
    int rc;
    if ((rc = ke_prepare(ctx, det, det_first, gt, gt_first, F, fr))) return rc;
    if (stage_ms) {
        for (hipEvent_t& e : ev.ev) PCR_HIP(ctx, hipEventCreate(&e));
        ev.on = true;
    }
    pcr_dev_block b_thr(ctx), b_n(ctx), b_counts(ctx);
    if ((rc = b_thr.alloc(sizeof(double) * KE_WORK)) || (rc = b_n.alloc(sizeof(int) * KE_COMBOS)) || (rc = b_counts.alloc(sizeof(unsigned long long) * 3 * KE_WORK))) return rc;
    if (ev.on) PCR_HIP(ctx, hipEventRecord(ev.ev[0], ctx->stream));
    if ((rc = ke_run_overlaps(ctx, fr, -1, 1))) return rc;
    if (ev.on) PCR_HIP(ctx, hipEventRecord(ev.ev[1], ctx->stream));
    if ((rc = ke_run_first(ctx, fr, mo, fi))) return rc;
    hipLaunchKernelGGL(ke_threshold_kernel, dim3(1), dim3(64), 0, ctx->stream, fi.sorted.as<const double>(), fi.d_begin(), (const unsigned int*)fi.d_end(),
                       fi.counts.as<const unsigned long long>(), b_thr.as<double>(), b_n.as<int>());
    PCR_HIP(ctx, hipGetLastError());
    if (ev.on) PCR_HIP(ctx, hipEventRecord(ev.ev[2], ctx->stream));
    if ((rc = ke_run_second(ctx, fr, mo, b_thr.as<const double>(), b_n.as<const int>(), b_counts.as<unsigned long long>()))) return rc;
    if (ev.on) PCR_HIP(ctx, hipEventRecord(ev.ev[3], ctx->stream));
    std::vector<double> h_thr((size_t)KE_WORK);
    std::vector<unsigned long long> h_counts((size_t)3 * KE_WORK);
    int h_n[KE_COMBOS];
    unsigned long long h_first[3 * KE_COMBOS];
    PCR_HIP(ctx, hipMemcpyAsync(h_thr.data(), b_thr.p, sizeof(double) * KE_WORK, hipMemcpyDeviceToHost, ctx->stream));
    PCR_HIP(ctx, hipMemcpyAsync(h_n, b_n.p, sizeof(h_n), hipMemcpyDeviceToHost, ctx->stream));
    PCR_HIP(ctx, hipMemcpyAsync(h_first, fi.counts.p, sizeof(h_first), hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = ke_download(ctx, h_counts.data(), b_counts.p, sizeof(unsigned long long) * h_counts.size()))) return rc;
    if (ev.on)
        for (int s = 0; s < 3; ++s) {
            float ms = 0.f;
            PCR_HIP(ctx, hipEventElapsedTime(&ms, ev.ev[s], ev.ev[s + 1]));
            stage_ms[s] = ms;
        }
    memset(result, 0, sizeof(*result));
    for (int cmd = 0; cmd < KE_COMBOS; ++cmd) {
        pcr_kitti_eval_cell& cell = result->cell[cmd / 9][(cmd / 3) % 3][cmd % 3];
        cell.n_gt = (int64_t)h_first[3 * cmd + 2];
        const int n = h_n[cmd] < 0 ? 0 : (h_n[cmd] > KE_S ? KE_S : h_n[cmd]);
        cell.n_thresholds = n;
        for (int k = 0; k < n; ++k) {
            const size_t j = (size_t)cmd * KE_S + k;
            cell.thresholds[k] = h_thr[j];
            const int64_t tp = (int64_t)h_counts[3 * j], fp = (int64_t)h_counts[3 * j + 1], fn = (int64_t)h_counts[3 * j + 2];
            cell.tp[k] = tp; cell.fp[k] = fp; cell.fn[k] = fn;
            cell.recall[k] = tp + fn != 0 ? (double)tp / (double)(tp + fn) : 0.0;
            cell.precision[k] = tp + fp != 0 ? (double)tp / (double)(tp + fp) : 0.0;
        }
        for (int k = KE_S - 2; k >= 0; --k)
            if (cell.precision[k + 1] > cell.precision[k]) cell.precision[k] = cell.precision[k + 1];
        double s11 = 0.0, s40 = 0.0;
        for (int k = 0; k < KE_S; k += 4) s11 += cell.precision[k];
        for (int k = 1; k < KE_S; ++k) s40 += cell.precision[k];
        cell.ap11 = 100.0 * (s11 / 11.0);
        cell.ap40 = 100.0 * (s40 / 40.0);
    }
    return PCR_OK;
} PCR_CATCH(ctx)

}  // extern "C"
