// The 64-row matrix-core MLP tile shared by the fused PointNet++ kernels (pcr_pointnet2_sa.hip: set abstraction, pcr_pointnet2_fp.hip:
// feature propagation): the tile's constants and the k loop of one 32-column stage.  Every output of a layer is ONE binary32 fmaf
// chain over k ascending (v_mfma_f32_32x32x2_f32: D = fma(a_k1, b_k1, fma(a_k0, b_k0, C)), each product rounded once), so both
// kernels are restated bit for bit by tests/sa_fused_checks.py.
#pragma once
#include "pcr_internal.h"

namespace {

constexpr int SA_TM = 64;        // rows per tile
constexpr int SA_KC = 32;        // columns of k per LDS stage
constexpr int SA_LDK = SA_KC + 1;   // odd row stride: the 32 lanes of an operand read (same k, 32 rows) hit 32 different banks
constexpr int SA_THREADS = 256;

typedef float sa_f32x16 __attribute__((ext_vector_type(16)));

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

}  // namespace
