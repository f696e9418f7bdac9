// The 64-row matrix-core MLP tile shared by the fused PointNet++ kernels (pcr_pointnet2_sa.hip: set abstraction, pcr_pointnet2_fp.hip:
// feature propagation): the tile's constants, the k loop of one 32-column stage, the loop over the layers of one tile
// (pn2_tile_layers) and, for the two entry points, the validation of a layer list and the choice of the width variant.  A kernel
// brings the expression for element (row, k) of layer 0 and what it does with the last activations; everything between is here, once.
//
// Arithmetic.  Every output of a layer is ONE binary32 fmaf chain over k ascending that starts at the bias, which is what
// v_mfma_f32_32x32x2_f32 computes: D = fma(a_k1, b_k1, fma(a_k0, b_k0, C)), each product rounded once, k0 the lanes 0..31 and k1 the
// lanes 32..63 of the operands.  The accumulator starts as the bias and one instruction after the other adds k = 2s, 2s + 1, so
// tests/sa_fused_checks.py restates both kernels bit for bit.  There is no split over k and no second chain per output.  The stored
// value is y = acc > 0 ? acc : +0, or acc + (+0) behind the last layer when relu_last is 0.
//
// Padding.  K is padded to the instruction's depth (2) and the widths to its tile (32) with zeros in BOTH operands:
//   - a padded k lies behind every real k (k >= K), so it can only change the END of the chain: fmaf(+0, +0, acc) = acc for every acc
//     except acc = -0, which becomes +0 (when K is odd).  The ReLU maps both zeros to +0, and without the last ReLU the explicit
//     acc + (+0) makes -0 -> +0 the rule for every K, so no stored bit depends on the padding.  (Zeros in the middle of a chain would
//     be as harmless -- a chain that passes through -0 meets a product that is not zero next, or ends -- but there are none.)
//   - a padded output channel has weights 0 and bias 0: its activation is +0, it is the padded k of the next layer (weights 0 there
//     too) and the kernels neither pool nor store it.
//   - a padded ROW (behind the last real row of a tile) is the kernel's: both give it a copy of the last real row, so it holds finite
//     data, and leave it out of what they pool or store.  Rows never mix: a row's outputs depend on that row alone.
//
// One tile.  64 rows x the layer's width, as 2 x width/32 blocks of 32 x 32 dealt to the four waves (block = wave + 4q has row half
// wave & 1 and channel tile (wave >> 1) + 2q, so the blocks of a wave share their A operand); the accumulators stay in registers.
//   layer 0   the rows come through LDS 32 columns at a time (K_0 is not bounded by LDS), beside the same 32 columns of the weights;
//   layer l   reads the previous activations from LDS (64 x width, row stride WMAX + 1), the weights again 32 columns at a time;
//   after the k loop of a layer nobody reads its input any more (one barrier), so the outputs overwrite it in place.
// A stage's weights and rows are fetched into registers while the stage before computes, and the k loop reads the next four steps'
// operands from LDS before it issues the current four: with one workgroup a CU nothing but the kernel's own order hides latency.
//
// Budget per WMAX = the largest width rounded up to 64 / 128 / 256.  LDS (floats): 64 * (WMAX + 1) activations + WMAX * 33 weights +
// 64 * 33 rows = 32.75 / 57 / 105.5 KiB, plus the kernel's per-row words (1 KiB in set abstraction, 3 KiB in feature propagation), of
// the CU's 160: four / two / one workgroup a CU by LDS.  Registers a lane: WMAX / 64 accumulator blocks of 16, WMAX / 8 + 8 for the
// stage fetched ahead, 8 * (1 + WMAX / 64) for the k loop's two operand sets; the compiler reports 32 / 64 / 128 AGPRs and some
// 90 / 145 / 235 VGPRs, which is 3 or 4 / 2 / 1 waves a SIMD, without scratch (profiles/pn2_layers_resources.md; a change here is
// checked against it: a variant that loses a wave or spills has lost the latency hiding the kernels were measured with).
#pragma once
#include <type_traits>
#include "pcr_internal.h"

namespace {

constexpr int SA_TM = 64;        // rows per tile
constexpr int SA_KC = 32;        // columns of k per LDS stage
constexpr int SA_LDK = SA_KC + 1;   // odd row stride: the 32 lanes of an operand read (same k, 32 rows) hit 32 different banks
constexpr int SA_THREADS = 256;

// what the tile holds on chip; include/pcr.h publishes the same figures once per entry point
constexpr int PN2_MAX_LAYERS = 3, PN2_MAX_WIDTH = 256, PN2_MAX_K0 = 1024;
static_assert(PCR_PN2_SA_MAX_LAYERS == PN2_MAX_LAYERS && PCR_PN2_SA_MAX_WIDTH == PN2_MAX_WIDTH && PCR_PN2_SA_MAX_K0 == PN2_MAX_K0, "pcr.h");
static_assert(PCR_PN2_FP_MAX_LAYERS == PN2_MAX_LAYERS && PCR_PN2_FP_MAX_WIDTH == PN2_MAX_WIDTH && PCR_PN2_FP_MAX_K0 == PN2_MAX_K0, "pcr.h");

typedef float sa_f32x16 __attribute__((ext_vector_type(16)));

// the folded layers of a call: layer l is N[l] x K[l] row-major weights and N[l] biases, K[0] the width of the kernel's rows and
// K[l] = N[l - 1]
struct pn2_layers {
    int n_layers;
    int K[PN2_MAX_LAYERS], N[PN2_MAX_LAYERS];
    const float* W[PN2_MAX_LAYERS];
    const float* bias[PN2_MAX_LAYERS];
};

// the k loop of one stage for a wave with NQ blocks: `steps` instructions per block, A from a_row (&A[this lane's row][its k half]),
// B from the weight stage (w_row: &s_w[this lane's channel of the wave's first block][k half]; block q: 64 channels further).  NQ is
// a compile-time count so that the loop unrolls and the LDS reads run ahead of the instructions that use them
template <int NQ, int QMAX>
__device__ static inline void sa_stage_steps(sa_f32x16 (&acc)[QMAX], int steps, const float* __restrict__ a_row, const float* __restrict__ w_row) {
    // groups of four steps, two register sets: the operands of the next group are read from LDS before the instructions of this one
    // are issued, so the read latency hides behind them (by hand: the optimizer declines to unroll or pipeline a loop of these
    // instructions with a run-time count).  The instructions of a block still issue in ascending k.
    float a0[4], w0[4][NQ], a1[4], w1[4][NQ];
    auto load = [&](float (&a)[4], float (&w)[4][NQ], int s) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            a[u] = a_row[2 * (s + u)];
#pragma unroll
            for (int q = 0; q < NQ; ++q) w[u][q] = w_row[q * 64 * SA_LDK + 2 * (s + u)];
        }
    };
    auto issue = [&](const float (&a)[4], const float (&w)[4][NQ]) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int q = 0; q < NQ; ++q) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], w[u][q], acc[q], 0, 0, 0);
    };
    int s = 0;
    if (steps >= 4) {
        load(a0, w0, 0);
        for (;;) {
            const bool more1 = s + 8 <= steps;
            if (more1) load(a1, w1, s + 4);
            issue(a0, w0);
            s += 4;
            if (!more1) break;
            const bool more0 = s + 8 <= steps;
            if (more0) load(a0, w0, s + 4);
            issue(a1, w1);
            s += 4;
            if (!more0) break;
        }
    }
    for (; s < steps; ++s) {
        const float a = a_row[2 * s];
#pragma unroll
        for (int q = 0; q < NQ; ++q) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, w_row[q * 64 * SA_LDK + 2 * s], acc[q], 0, 0, 0);
    }
}
template <int QMAX>
__device__ static inline void sa_stage_mfma(sa_f32x16 (&acc)[QMAX], int nq, int steps, const float* __restrict__ a_row, const float* __restrict__ w_row) {
    // (nq is wave-uniform and at most QMAX; the conditional template arguments only keep the branches that cannot be taken compilable)
    if (nq == 1) sa_stage_steps<1, QMAX>(acc, steps, a_row, w_row);
    if (QMAX >= 2 && nq == 2) sa_stage_steps<(QMAX >= 2 ? 2 : 1), QMAX>(acc, steps, a_row, w_row);
    if (QMAX >= 4 && nq == 3) sa_stage_steps<(QMAX >= 4 ? 3 : 1), QMAX>(acc, steps, a_row, w_row);
    if (QMAX >= 4 && nq == 4) sa_stage_steps<(QMAX >= 4 ? 4 : 1), QMAX>(acc, steps, a_row, w_row);
}

// All layers of one 64-row tile, by the 256 threads of a workgroup.  row0(r, k) is element k < K[0] of tile row r < 64 of layer 0
// (never called for a padded k).  s_act[64 * (WMAX + 1)], s_w[WMAX * 33], s_x[64 * 33] are the workgroup's LDS; whatever row0 reads
// from LDS must have been written in front of a barrier.  On return the last layer's outputs are in s_act (row stride WMAX + 1,
// channels < N[n_layers - 1]) behind a barrier; relu_last false stores the last layer as acc + (+0).  Forced inline: s_act, s_w and
// s_x are LDS addresses only inside the kernel, and a kernel that always wants the last ReLU passes the literal, which folds the
// other form away (as a run-time word it cost the set-abstraction modules 0.5 to 2 % of their time).
template <int WMAX, class Row0>
__device__ __forceinline__ void pn2_tile_layers(const pn2_layers& p, bool relu_last, float* s_act, float* s_w, float* s_x, Row0 row0) {
    constexpr int LDA = WMAX + 1;
    constexpr int QMAX = WMAX / 64;                  // blocks per wave: 2 * (WMAX / 32) blocks over four waves
    constexpr int WREGS = WMAX * SA_KC / SA_THREADS, XREGS = SA_TM * SA_KC / SA_THREADS;   // a stage's elements per thread
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, half = lane >> 5;
    const int rb = wave & 1, cb0 = wave >> 1;        // this wave's row half and first channel tile

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
        // A stage's weights s_w[channel][kk] (zeros behind N and behind K) and, for layer 0, its rows are read from memory into
        // registers one stage AHEAD, while the matrix instructions of the stage before run, and go to LDS behind that stage's
        // barrier: thread t holds elements t, t + 256, ... of a stage, element e = (channel or row e >> 5, column e & 31).
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
                for (int i = 0; i < XREGS; ++i) xreg[i] = kk < kw ? row0((tid >> 5) + 8 * i, kc + kk) : 0.0f;
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
        // the outputs in place of the layer's input.  Register e of a lane is row (e & 3) + 8 (e >> 2) + 4 half of the block, the
        // lane's channel is l31 (the C/D map of the 32 x 32 instructions)
        const bool relu = relu_last || l + 1 < p.n_layers;
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
}

// ---- host: what the two entry points do with a layer list

// Every status an entry point returns before its grid-size check, in the ABI's order: PCR_E_INVALID (the entry point's own argument
// test `args_ok` -- sizes, and for a call that is not empty its pointers --, the layer count, K_0, a width below 1, and for a call
// that is not empty the layer arrays and every layer's pointers), then PCR_E_UNSUPPORTED for layers / K_0 / width, then PCR_OK:
// with `empty` nothing else happens and the caller returns; otherwise `lay` is filled and *wmax is the largest width.  All the
// PCR_E_INVALID tests are free of side effects and give one status, so which of them runs first cannot be observed.
inline int pn2_layers_from(bool args_ok, bool empty, long long k0, int n_layers, const int* widths, const float* const* weights,
                           const float* const* biases, pn2_layers* lay, int* wmax) {
    if (!args_ok || n_layers < 1 || !widths || k0 < 1) return PCR_E_INVALID;
    for (int l = 0; l < n_layers; ++l)
        if (widths[l] < 1) return PCR_E_INVALID;
    if (!empty) {
        if (!weights || !biases) return PCR_E_INVALID;
        for (int l = 0; l < n_layers && l < PN2_MAX_LAYERS; ++l)
            if (!weights[l] || !biases[l]) return PCR_E_INVALID;
    }
    if (n_layers > PN2_MAX_LAYERS || k0 > PN2_MAX_K0) return PCR_E_UNSUPPORTED;
    *wmax = 0;
    for (int l = 0; l < n_layers; ++l) {
        if (widths[l] > PN2_MAX_WIDTH) return PCR_E_UNSUPPORTED;
        *wmax = widths[l] > *wmax ? widths[l] : *wmax;
    }
    if (empty) return PCR_OK;
    lay->n_layers = n_layers;
    for (int l = 0; l < PN2_MAX_LAYERS; ++l) {
        const bool on = l < n_layers;
        lay->K[l] = !on ? 0 : l == 0 ? (int)k0 : widths[l - 1];
        lay->N[l] = on ? widths[l] : 0;
        lay->W[l] = on ? weights[l] : nullptr;
        lay->bias[l] = on ? biases[l] : nullptr;
    }
    return PCR_OK;
}

// launch(std::integral_constant<int, WMAX>) for the smallest variant that holds wmax -> PCR_OK or PCR_E_HIP
template <class Launch>
inline int pn2_launch_for_width(int wmax, Launch launch) {
    if (wmax <= 64) launch(std::integral_constant<int, 64>());
    else if (wmax <= 128) launch(std::integral_constant<int, 128>());
    else launch(std::integral_constant<int, 256>());
    return hipGetLastError() == hipSuccess ? PCR_OK : PCR_E_HIP;
}

}  // namespace
