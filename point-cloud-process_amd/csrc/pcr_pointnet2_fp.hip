// PointNet++ feature propagation for inference, fused (include/pcr.h, pcr_pn2_fp_mlp): build every point's row -- the three-point
// interpolation of the known points' features, then the point's own (skip) features -- and run the per-point shared MLP with the batch
// norm folded into its weights.  The interpolated tensor, the (b, C2 + C1, n) concatenation and the convolution / batch norm / ReLU
// intermediates never exist in memory.  Device pointers in, one kernel on the caller's stream, no context, no allocation, no wait.
// The neighbour search and the weights are the caller's (three_nn and three small tensor ops): the kernel starts from idx and weight.
//
// Arithmetic.  An interpolated entry is ((p0*w0) + (p1*w1)) + (p2*w2) in binary32 without contraction, the expression of
// pcr_pn2_three_interpolate.  The layers are those of pcr_pointnet2_sa.hip: every output ONE binary32 fmaf chain over k ascending that
// starts at the bias (the k loop is the shared one of pcr_pn2_mlp_tile.h), ReLU as acc > 0 ? acc : +0.  Without the last ReLU the
// stored value is acc + (+0): K is padded to the instruction's depth (2) with zeros in both operands BEHIND every real k, which turns
// an accumulator of -0 into +0 when K is odd; the explicit addition makes that the rule for every K.
//
// Tiling.  Four waves own 64 consecutive rows of the b*n rows (a tile may straddle two clouds, so the cloud and the point of a row
// are kept per row in LDS beside its three source rows bi*m + idx and its three weights); a row belongs to exactly one workgroup, so
// every out[bi, j, i] is stored once, without atomics or zeroing.  Rows of the last tile that stand for no point are copies of the
// last real row and are never stored.
//   layer 0   the rows come through LDS 32 columns at a time: a thread's column of a stage reads three contiguous 128-byte pieces of
//             known_feats (k < c_known) or one of skip_feats; a stage may contain the c_known boundary;
//   layer l   as in sa_mlp_max_kernel: activations in LDS (64 x width, row stride width + 1), overwritten in place behind a barrier;
//   store     lanes along the rows: a wave stores 64 consecutive i of one channel (256 bytes), and the odd row stride of the
//             activations puts the 32 lanes of a half-wave on 32 different banks.
// LDS (floats): 64 * (W + 1) activations + W * 33 weights + 64 * 33 rows + 3 KiB of per-row words, W = 64 / 128 / 256: 36 / 60 /
// 109 KiB of the CU's 160, so two workgroups a CU up to width 128 and one at 256; registers as in the set-abstraction kernel.
#include "pcr_internal.h"
#include "pcr_pn2_mlp_tile.h"

namespace {

constexpr int FP_MAX_LAYERS = PCR_PN2_FP_MAX_LAYERS;

struct fp_args {
    int n, m, c_known, c_skip, n_layers, relu_last;
    long long rows;                    // b * n
    int K[FP_MAX_LAYERS], N[FP_MAX_LAYERS];
    const float* W[FP_MAX_LAYERS];
    const float* bias[FP_MAX_LAYERS];
    const float* known;
    const int* idx;
    const float* weight;
    const float* skip;
    float* out;
};

template <int WMAX>
__global__ __launch_bounds__(SA_THREADS) void fp_mlp_kernel(const fp_args p) {
    constexpr int LDA = WMAX + 1;
    constexpr int QMAX = WMAX / 64;                  // blocks per wave: 2 * (WMAX / 32) blocks over four waves
    constexpr int WREGS = WMAX * SA_KC / SA_THREADS, XREGS = SA_TM * SA_KC / SA_THREADS;   // a stage's elements per thread
    __shared__ float s_act[SA_TM * LDA];
    __shared__ float s_w[WMAX * SA_LDK];
    __shared__ float s_x[SA_TM * SA_LDK];
    __shared__ long long s_src[3][SA_TM];            // row -> bi * m + idx[bi, i, j]
    __shared__ float s_wt[3][SA_TM];                 // row -> weight[bi, i, j]
    __shared__ long long s_row[SA_TM];               // row -> bi * n + i
    __shared__ long long s_dst[SA_TM];               // row -> bi * c_last * n + i: element (bi, 0, i) of out

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, half = lane >> 5;
    const long long r0 = (long long)blockIdx.x * SA_TM;
    const int valid = (int)(p.rows - r0 < SA_TM ? p.rows - r0 : (long long)SA_TM);
    const int c_last = p.N[p.n_layers - 1];
    // blocks of 32 rows x 32 channels: block = wave + 4q has row half (wave & 1) and channel tile (wave >> 1) + 2q
    const int rb = wave & 1, cb0 = wave >> 1;

    if (tid < SA_TM) {
        const long long g = r0 + (tid < valid ? tid : valid - 1);     // behind the end: a copy of the last real row
        const long long bi = g / p.n, i = g - bi * p.n;
        s_row[tid] = g;
        s_dst[tid] = bi * c_last * p.n + i;
        if (p.c_known > 0) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                s_src[j][tid] = bi * p.m + p.idx[g * 3 + j];
                s_wt[j][tid] = p.weight[g * 3 + j];
            }
        }
    }
    __syncthreads();

    for (int l = 0; l < p.n_layers; ++l) {
        const int K = p.K[l], N = p.N[l];
        const int npad = (N + 31) & ~31;
        const int nq = (npad / 32 - cb0 + 1) / 2;                     // this wave's blocks: channel tiles cb0, cb0 + 2, ... < npad / 32
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
        // A stage's weights s_w[channel][kk] (zeros behind N and behind K) and, for layer 0, its rows (the interpolated entries, then
        // the skip features) are read from memory into registers one stage AHEAD, while the matrix instructions of the stage before
        // run, and go to LDS behind that stage's barrier: thread t holds elements t, t + 256, ... of a stage, element
        // e = (channel or row e >> 5, column e & 31).
        float wreg[WREGS], xreg[XREGS];
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
                        if (k < p.c_known) {
                            const float p0 = p.known[s_src[0][r] * p.c_known + k], p1 = p.known[s_src[1][r] * p.c_known + k],
                                        p2 = p.known[s_src[2][r] * p.c_known + k];
                            v = ((p0 * s_wt[0][r]) + (p1 * s_wt[1][r])) + (p2 * s_wt[2][r]);
                        } else {
                            v = p.skip[s_row[r] * p.c_skip + (k - p.c_known)];
                        }
                    }
                    xreg[i] = v;
                }
            }
        };
        fetch(0);
        for (int kc = 0; kc < K; kc += SA_KC) {
            const int kw = K - kc < SA_KC ? K - kc : SA_KC;           // real columns of this stage
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
            __syncthreads();                                          // the stage is free again; after the last one: so is s_act
        }
        // y = acc > 0 ? acc : +0 (or acc + (+0) behind the last layer without ReLU) in place of the layer's input.  Register e of a
        // lane is row (e & 3) + 8 (e >> 2) + 4 half of the block, the lane's channel is l31 (the C/D map of the 32 x 32 instructions)
        const bool relu = l + 1 < p.n_layers || p.relu_last != 0;
#pragma unroll
        for (int q = 0; q < QMAX; ++q) {
            if (q < nq) {
                float* dst = s_act + (rb * 32 + 4 * half) * LDA + (cb0 + 2 * q) * 32 + l31;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const float v = acc[q][e];
                    dst[((e & 3) + 8 * (e >> 2)) * LDA] = relu ? (v > 0.0f ? v : 0.0f) : v + 0.0f;
                }
            }
        }
        __syncthreads();
    }

    // the last activations, lanes along the rows: wave w stores channels w, w + 4, ...; real rows only
    if (lane < valid) {
        float* dst = p.out + s_dst[lane];
        const float* src = s_act + lane * LDA;
        for (int j = wave; j < c_last; j += SA_THREADS / 64) dst[(long long)j * p.n] = src[j];
    }
}

template <int WMAX>
static hipError_t fp_launch(hipStream_t s, unsigned int blocks, const fp_args& a) {
    hipLaunchKernelGGL((fp_mlp_kernel<WMAX>), dim3(blocks), dim3(SA_THREADS), 0, s, a);
    return hipGetLastError();
}

}  // namespace

extern "C" int pcr_pn2_fp_mlp(void* stream, int b, int n, int m, int c_known, int c_skip, const float* known_feats, const int32_t* idx,
                              const float* weight, const float* skip_feats, int n_layers, const int* widths, const float* const* weights,
                              const float* const* biases, int relu_last, float* out) {
    if (b < 0 || n < 0 || m < 0 || c_known < 0 || c_skip < 0 || n_layers < 1 || !widths) return PCR_E_INVALID;
    const long long k0 = (long long)c_known + c_skip;
    if (k0 < 1) return PCR_E_INVALID;
    for (int l = 0; l < n_layers; ++l)
        if (widths[l] < 1) return PCR_E_INVALID;
    const bool empty = b == 0 || n == 0;
    if (!empty && (!weights || !biases || !out || (c_known > 0 && (m < 1 || !known_feats || !idx || !weight)) || (c_skip > 0 && !skip_feats)))
        return PCR_E_INVALID;
    if (!empty)
        for (int l = 0; l < n_layers && l < FP_MAX_LAYERS; ++l)
            if (!weights[l] || !biases[l]) return PCR_E_INVALID;
    if (n_layers > PCR_PN2_FP_MAX_LAYERS || k0 > PCR_PN2_FP_MAX_K0) return PCR_E_UNSUPPORTED;
    int wmax = 0;
    for (int l = 0; l < n_layers; ++l) {
        if (widths[l] > PCR_PN2_FP_MAX_WIDTH) return PCR_E_UNSUPPORTED;
        wmax = widths[l] > wmax ? widths[l] : wmax;
    }
    if (empty) return PCR_OK;
    fp_args a;
    a.n = n; a.m = m; a.c_known = c_known; a.c_skip = c_skip; a.n_layers = n_layers; a.relu_last = relu_last ? 1 : 0;
    a.rows = (long long)b * n;
    for (int l = 0; l < FP_MAX_LAYERS; ++l) {
        const bool on = l < n_layers;
        a.K[l] = !on ? 0 : l == 0 ? (int)k0 : widths[l - 1];
        a.N[l] = on ? widths[l] : 0;
        a.W[l] = on ? weights[l] : nullptr;
        a.bias[l] = on ? biases[l] : nullptr;
    }
    a.known = known_feats; a.idx = idx; a.weight = weight; a.skip = skip_feats; a.out = out;
    const long long tiles = (a.rows + SA_TM - 1) / SA_TM;
    if (tiles > 0x7FFFFFFF) return PCR_E_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = wmax <= 64 ? fp_launch<64>(s, (unsigned int)tiles, a) : wmax <= 128 ? fp_launch<128>(s, (unsigned int)tiles, a)
                                                                                              : fp_launch<256>(s, (unsigned int)tiles, a);
    return e == hipSuccess ? PCR_OK : PCR_E_HIP;
}
