// PointNet++ set abstraction for inference, fused (include/pcr.h, pcr_pn2_sa_mlp_max): gather the ball's rows, run the shared MLP with
// the batch norm folded into its weights, ReLU, and keep the maximum over the ball -- the grouped tensor (b, C, m, nsample) never
// exists in memory.  Device pointers in, one kernel on the caller's stream, no context, no allocation, no wait.
//
// Arithmetic.  Every output of a layer is ONE binary32 fmaf chain over k ascending that starts at the bias, which is what
// v_mfma_f32_32x32x2_f32 computes: D = fma(a_k1, b_k1, fma(a_k0, b_k0, C)), each product rounded once, k0 the lanes 0..31 and k1 the
// lanes 32..63 of the operands.  The accumulator starts as the bias and one instruction after the other adds k = 2s, 2s + 1, so
// tests/sa_fused_checks.py restates the kernel bit for bit.  There is no split over k and no second chain per output.
//
// Padding.  K is padded to the instruction's depth (2) and the widths to its tile (32) with zeros in BOTH operands:
//   - a padded k lies behind every real k (k >= K), so it can only change the END of the chain: fmaf(+0, +0, acc) = acc for every acc
//     except acc = -0, which becomes +0; the ReLU that follows maps both zeros to +0, so no output bit changes.  (Zeros in the middle
//     of a chain would be as harmless -- a chain that passes through -0 meets a product that is not zero next, or ends -- but there
//     are none.)
//   - a padded output channel has weights 0 and bias 0: its activation is +0, it is the padded k of the next layer (weights 0 there
//     too) and it is never pooled.
//   - a padded ROW (the last tile of a unit) gathers a copy of the unit's last real row, so it holds finite data, and the pooling
//     loop runs over real rows only: it can never win a maximum.
//
// Tiling.  A workgroup of four waves owns a UNIT: G = 64 / nsample whole centres when nsample <= 64, one centre otherwise, and walks
// the unit's rows 64 at a time.  So no two workgroups ever share a centre: one plain store per (channel, centre), no atomics, no
// zeroing of `out`.  Per tile of 64 rows:
//   layer 0   the gathered rows come through LDS 32 columns at a time (K_0 is not bounded by LDS), beside the same 32 columns of the
//             weights; the accumulators of the whole 64 x width tile stay in registers (2 x width/32 blocks of 32 x 32, dealt to
//             the four waves: at most four blocks = 64 registers a lane at width 256);
//   layer l   reads the previous activations from LDS (64 x width, row stride width + 1), the weights again 32 columns at a time;
//   after the k loop of a layer nobody reads its input any more (one barrier), so the ReLU'd outputs overwrite it in place;
//   pooling   one thread per (centre, channel) takes the maximum over the centre's rows of the tile; a centre of more than 64 rows
//             keeps its running maximum in the register of thread `channel` across its tiles.
// LDS (floats): 64 * (W + 1) activations + W * 33 weights + 64 * 33 gathered rows, W = the largest width rounded up to
// 64 / 128 / 256: 34 / 58 / 107 KiB of the CU's 160, so two workgroups a CU up to width 128 and one at 256.  With one workgroup a CU
// nothing but the kernel's own order hides latency: a stage's weights and rows are fetched into registers while the stage before
// computes, and the k loop reads the next four steps' operands from LDS before it issues the current four.
#include "pcr_internal.h"
#include "pcr_pn2_mlp_tile.h"   // the tile's constants and the k loop of a stage (sa_stage_mfma), shared with pcr_pointnet2_fp.hip

namespace {

constexpr int SA_MAX_LAYERS = 3;

struct sa_args {
    int n, m, nsample, c_feat, use_xyz, n_layers;
    int group;                         // centres per unit
    long long centres;                 // b * m
    long long out_batch_stride;
    int K[SA_MAX_LAYERS], N[SA_MAX_LAYERS];
    const float* W[SA_MAX_LAYERS];
    const float* bias[SA_MAX_LAYERS];
    const float* xyz;
    const float* new_xyz;
    const float* feats;
    const int* idx;
    float* out;
};

template <int WMAX>
__global__ __launch_bounds__(SA_THREADS) void sa_mlp_max_kernel(const sa_args p) {
    constexpr int LDA = WMAX + 1;
    constexpr int QMAX = WMAX / 64;                  // blocks per wave: 2 * (WMAX / 32) blocks over four waves
    constexpr int WREGS = WMAX * SA_KC / SA_THREADS, XREGS = SA_TM * SA_KC / SA_THREADS;   // a stage's elements per thread
    __shared__ float s_act[SA_TM * LDA];
    __shared__ float s_w[WMAX * SA_LDK];
    __shared__ float s_x[SA_TM * SA_LDK];
    __shared__ long long s_pt[SA_TM];                // row -> bi * n + point
    __shared__ long long s_cg[SA_TM];                // row -> bi * m + centre

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, half = lane >> 5;
    const long long c0 = (long long)blockIdx.x * p.group;                                   // first centre of the unit
    const int gt = (int)(p.centres - c0 < p.group ? p.centres - c0 : (long long)p.group);   // its centres
    const int unit_rows = gt * p.nsample;
    const int c_last = p.N[p.n_layers - 1];
    // blocks of 32 rows x 32 channels: block = wave + 4q has row half (wave & 1) and channel tile (wave >> 1) + 2q
    const int rb = wave & 1, cb0 = wave >> 1;
    float run = 0.0f;                                // (group == 1) running maximum of channel `tid`

    for (int r0 = 0; r0 < unit_rows; r0 += SA_TM) {
        const int valid = unit_rows - r0 < SA_TM ? unit_rows - r0 : SA_TM;
        if (tid < SA_TM) {
            const int r = r0 + (tid < valid ? tid : valid - 1);       // behind the end: a copy of the last real row
            const int g = r / p.nsample;
            const long long cg = c0 + g, bi = cg / p.m;
            s_cg[tid] = cg;
            s_pt[tid] = bi * p.n + p.idx[cg * p.nsample + (r - g * p.nsample)];
        }
        __syncthreads();

        for (int l = 0; l < p.n_layers; ++l) {
            const int K = p.K[l], N = p.N[l];
            const int npad = (N + 31) & ~31;
            const int nq = (npad / 32 - cb0 + 1) / 2;                 // this wave's blocks: channel tiles cb0, cb0 + 2, ... < npad / 32
            const float* __restrict__ W = p.W[l];
            const float* __restrict__ bias = p.bias[l];
            sa_f32x16 acc[QMAX];
#pragma unroll
            for (int q = 0; q < QMAX; ++q) {
                const int ch = (cb0 + 2 * q) * 32 + l31;
                const float b0 = (q < nq && ch < N) ? bias[ch] : 0.0f;
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[q][e] = b0;
            }
            // A stage's weights s_w[channel][kk] (zeros behind N and behind K) and, for layer 0, its gathered rows (relative coordinates
            // first with use_xyz, then the point's features) are read from memory into registers one stage AHEAD, while the matrix
            // instructions of the stage before run, and go to LDS behind that stage's barrier: thread t holds elements t, t + 256, ...
            // of a stage, element e = (channel or row e >> 5, column e & 31).
            float wreg[WREGS], xreg[XREGS];
            const int xo = p.use_xyz ? 3 : 0;
            auto fetch = [&](int kc) {
                const int kw = K - kc < SA_KC ? K - kc : SA_KC;
                const int kk = tid & 31;
#pragma unroll
                for (int i = 0; i < WREGS; ++i) {
                    const int j = (tid >> 5) + 8 * i;
                    wreg[i] = (j < N && kk < kw) ? W[(long long)j * K + kc + kk] : 0.0f;
                }
                if (l == 0) {
#pragma unroll
                    for (int i = 0; i < XREGS; ++i) {
                        const int r = (tid >> 5) + 8 * i, k = kc + kk;
                        float v = 0.0f;
                        if (kk < kw) {
                            if (k < xo) v = p.xyz[s_pt[r] * 3 + k] - p.new_xyz[s_cg[r] * 3 + k];
                            else v = p.feats[s_pt[r] * p.c_feat + (k - xo)];
                        }
                        xreg[i] = v;
                    }
                }
            };
            fetch(0);
            for (int kc = 0; kc < K; kc += SA_KC) {
                const int kw = K - kc < SA_KC ? K - kc : SA_KC;       // real columns of this stage
#pragma unroll
                for (int i = 0; i < WREGS; ++i) {
                    const int j = (tid >> 5) + 8 * i;
                    if (j < npad) s_w[j * SA_LDK + (tid & 31)] = wreg[i];
                }
                if (l == 0) {
#pragma unroll
                    for (int i = 0; i < XREGS; ++i) s_x[((tid >> 5) + 8 * i) * SA_LDK + (tid & 31)] = xreg[i];
                }
                __syncthreads();
                if (kc + SA_KC < K) fetch(kc + SA_KC);
                const float* a_row = l == 0 ? s_x + (rb * 32 + l31) * SA_LDK + half : s_act + (rb * 32 + l31) * LDA + kc + half;
                sa_stage_mfma<QMAX>(acc, nq, (kw + 1) >> 1, a_row, s_w + (cb0 * 32 + l31) * SA_LDK + half);
                __syncthreads();                                      // the stage is free again; after the last one: so is s_act
            }
            // y = acc > 0 ? acc : +0 in place of the layer's input.  Register e of a lane is row (e & 3) + 8 (e >> 2) + 4 half of the
            // block, the lane's channel is l31 (the C/D map of the 32 x 32 instructions)
#pragma unroll
            for (int q = 0; q < QMAX; ++q) {
                if (q < nq) {
                    float* dst = s_act + (rb * 32 + 4 * half) * LDA + (cb0 + 2 * q) * 32 + l31;
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const float v = acc[q][e];
                        dst[((e & 3) + 8 * (e >> 2)) * LDA] = v > 0.0f ? v : 0.0f;
                    }
                }
            }
            __syncthreads();
        }

        // the maximum over each centre's rows of this tile (every y is >= +0, so 0 is the identity)
        if (p.group == 1) {
            if (tid < c_last)
                for (int r = 0; r < valid; ++r) {
                    const float v = s_act[r * LDA + tid];
                    run = v > run ? v : run;
                }
        } else {
            for (int e = tid; e < gt * c_last; e += SA_THREADS) {
                const int g = e / c_last, j = e - g * c_last;
                float best = 0.0f;
                for (int r = g * p.nsample; r < (g + 1) * p.nsample; ++r) {
                    const float v = s_act[r * LDA + j];
                    best = v > best ? v : best;
                }
                const long long cg = c0 + g, bi = cg / p.m;
                p.out[bi * p.out_batch_stride + (long long)j * p.m + (cg - bi * p.m)] = best;
            }
        }
        __syncthreads();                                              // the next tile overwrites s_pt, s_cg and s_act
    }
    if (p.group == 1 && tid < c_last) {
        const long long bi = c0 / p.m;
        p.out[bi * p.out_batch_stride + (long long)tid * p.m + (c0 - bi * p.m)] = run;
    }
}

template <int WMAX>
static hipError_t sa_launch(hipStream_t s, unsigned int blocks, const sa_args& a) {
    hipLaunchKernelGGL((sa_mlp_max_kernel<WMAX>), dim3(blocks), dim3(SA_THREADS), 0, s, a);
    return hipGetLastError();
}

}  // namespace

extern "C" int pcr_pn2_sa_mlp_max(void* stream, int b, int n, int m, int nsample, int c_feat, int use_xyz, const float* xyz, const float* new_xyz,
                                  const float* feats, const int32_t* idx, int n_layers, const int* widths, const float* const* weights,
                                  const float* const* biases, float* out, long long out_batch_stride) {
    if (b < 0 || n < 0 || m < 0 || nsample < 0 || c_feat < 0 || c_feat > 0x7FFFFFFF - 3 || n_layers < 1 || !widths) return PCR_E_INVALID;
    const int k0 = (use_xyz ? 3 : 0) + c_feat;
    if (k0 < 1) return PCR_E_INVALID;
    for (int l = 0; l < n_layers; ++l)
        if (widths[l] < 1) return PCR_E_INVALID;
    const bool empty = b == 0 || m == 0;
    if (!empty && (nsample < 1 || n < 1 || !weights || !biases || !idx || !out || (use_xyz && (!xyz || !new_xyz)) || (c_feat > 0 && !feats) ||
                   out_batch_stride < 0))
        return PCR_E_INVALID;
    if (!empty)
        for (int l = 0; l < n_layers && l < SA_MAX_LAYERS; ++l)
            if (!weights[l] || !biases[l]) return PCR_E_INVALID;
    if (n_layers > PCR_PN2_SA_MAX_LAYERS || k0 > PCR_PN2_SA_MAX_K0) return PCR_E_UNSUPPORTED;
    int wmax = 0;
    for (int l = 0; l < n_layers; ++l) {
        if (widths[l] > PCR_PN2_SA_MAX_WIDTH) return PCR_E_UNSUPPORTED;
        wmax = widths[l] > wmax ? widths[l] : wmax;
    }
    if (empty) return PCR_OK;
    sa_args a;
    a.n = n; a.m = m; a.nsample = nsample; a.c_feat = c_feat; a.use_xyz = use_xyz ? 1 : 0; a.n_layers = n_layers;
    a.group = nsample <= SA_TM ? SA_TM / nsample : 1;
    a.centres = (long long)b * m;
    a.out_batch_stride = out_batch_stride;
    for (int l = 0; l < SA_MAX_LAYERS; ++l) {
        const bool on = l < n_layers;
        a.K[l] = !on ? 0 : l == 0 ? k0 : widths[l - 1];
        a.N[l] = on ? widths[l] : 0;
        a.W[l] = on ? weights[l] : nullptr;
        a.bias[l] = on ? biases[l] : nullptr;
    }
    a.xyz = xyz; a.new_xyz = new_xyz; a.feats = feats; a.idx = idx; a.out = out;
    const long long units = (a.centres + a.group - 1) / a.group;
    if (units > 0x7FFFFFFF) return PCR_E_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = wmax <= 64 ? sa_launch<64>(s, (unsigned int)units, a) : wmax <= 128 ? sa_launch<128>(s, (unsigned int)units, a)
                                                                                              : sa_launch<256>(s, (unsigned int)units, a);
    return e == hipSuccess ? PCR_OK : PCR_E_HIP;
}
