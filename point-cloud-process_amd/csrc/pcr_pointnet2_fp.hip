// PointNet++ feature propagation for inference, fused (include/pcr.h, pcr_pn2_fp_mlp): build every point's row -- the three-point
// interpolation of the known points' features, then the point's own (skip) features -- and run the per-point shared MLP with the batch
// norm folded into its weights.  The interpolated tensor, the (b, C2 + C1, n) concatenation and the convolution / batch norm / ReLU
// intermediates never exist in memory.  Device pointers in, one kernel on the caller's stream, no context, no allocation, no wait.
// The neighbour search and the weights are the caller's (three_nn and three small tensor ops): the kernel starts from idx and weight.
//
// Arithmetic.  An interpolated entry is ((p0*w0) + (p1*w1)) + (p2*w2) in binary32 without contraction, the expression of
// pcr_pn2_three_interpolate; a skip entry is the feature as stored.  The layers, their padding, the acc + (+0) rule without the last
// ReLU and why no stored bit depends on the padding are pcr_pn2_mlp_tile.h's (pn2_tile_layers).
//
// Tiling.  Four waves own 64 consecutive rows of the b*n rows (a tile may straddle two clouds, so the cloud and the point of a row
// are kept per row in LDS beside its three source rows bi*m + idx and its three weights); a row belongs to exactly one workgroup, so
// every out[bi, j, i] is stored once, without atomics or zeroing.  Rows of the last tile that stand for no point are copies of the
// last real row and are never stored.
//   layer 0   a thread's column of a 32-column stage reads three contiguous 128-byte pieces of known_feats (k < c_known) or one of
//             skip_feats; a stage may contain the c_known boundary;
//   layers    pn2_tile_layers, which leaves the last activations in LDS (64 x width, row stride WMAX + 1);
//   store     lanes along the rows: a wave stores 64 consecutive i of one channel (256 bytes), and the odd row stride of the
//             activations puts the 32 lanes of a half-wave on 32 different banks.
// LDS and registers per variant: the shared header's budget plus 3 KiB of per-row words, 36 / 60.25 / 108.75 KiB of the CU's 160.
#include "pcr_internal.h"
#include "pcr_pn2_mlp_tile.h"

namespace {

struct fp_args {
    int n, m, c_known, c_skip, relu_last;
    long long rows;                    // b * n
    pn2_layers layers;
    const float* known;
    const int* idx;
    const float* weight;
    const float* skip;
    float* out;
};

template <int WMAX>
__global__ __launch_bounds__(SA_THREADS) void fp_mlp_kernel(const fp_args p) {
    constexpr int LDA = WMAX + 1;
    __shared__ float s_act[SA_TM * LDA];
    __shared__ float s_w[WMAX * SA_LDK];
    __shared__ float s_x[SA_TM * SA_LDK];
    __shared__ long long s_src[3][SA_TM];            // row -> bi * m + idx[bi, i, j]
    __shared__ float s_wt[3][SA_TM];                 // row -> weight[bi, i, j]
    __shared__ long long s_row[SA_TM];               // row -> bi * n + i
    __shared__ long long s_dst[SA_TM];               // row -> bi * c_last * n + i: element (bi, 0, i) of out

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long r0 = (long long)blockIdx.x * SA_TM;
    const int valid = (int)(p.rows - r0 < SA_TM ? p.rows - r0 : (long long)SA_TM);
    const int c_last = p.layers.N[p.layers.n_layers - 1];

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

    // element k of row r: the interpolated entries, then the skip features
    pn2_tile_layers<WMAX>(p.layers, p.relu_last != 0, s_act, s_w, s_x, [&](int r, int k) {
        if (k >= p.c_known) return p.skip[s_row[r] * p.c_skip + (k - p.c_known)];
        const float p0 = p.known[s_src[0][r] * p.c_known + k], p1 = p.known[s_src[1][r] * p.c_known + k], p2 = p.known[s_src[2][r] * p.c_known + k];
        return ((p0 * s_wt[0][r]) + (p1 * s_wt[1][r])) + (p2 * s_wt[2][r]);
    });

    // the last activations, lanes along the rows: wave w stores channels w, w + 4, ...; real rows only
    if (lane < valid) {
        float* dst = p.out + s_dst[lane];
        const float* src = s_act + lane * LDA;
        for (int j = wave; j < c_last; j += SA_THREADS / 64) dst[(long long)j * p.n] = src[j];
    }
}

}  // namespace

extern "C" int pcr_pn2_fp_mlp(void* stream, int b, int n, int m, int c_known, int c_skip, const float* known_feats, const int32_t* idx,
                              const float* weight, const float* skip_feats, int n_layers, const int* widths, const float* const* weights,
                              const float* const* biases, int relu_last, float* out) {
    const bool empty = b == 0 || n == 0;
    // the sizes; for a call that is not empty, every pointer the kernel would read or write
    const bool args_ok = b >= 0 && n >= 0 && m >= 0 && c_known >= 0 && c_skip >= 0 &&
                         (empty || (out && (c_known == 0 || (m >= 1 && known_feats && idx && weight)) && (c_skip == 0 || skip_feats)));
    fp_args a;
    int wmax = 0;
    const int st = pn2_layers_from(args_ok, empty, (long long)c_known + c_skip, n_layers, widths, weights, biases, &a.layers, &wmax);
    if (st != PCR_OK || empty) return st;
    a.n = n; a.m = m; a.c_known = c_known; a.c_skip = c_skip; a.relu_last = relu_last ? 1 : 0;
    a.rows = (long long)b * n;
    a.known = known_feats; a.idx = idx; a.weight = weight; a.skip = skip_feats; a.out = out;
    const long long tiles = (a.rows + SA_TM - 1) / SA_TM;
    if (tiles > 0x7FFFFFFF) return PCR_E_UNSUPPORTED;
    return pn2_launch_for_width(wmax, [&](auto w) {
        hipLaunchKernelGGL((fp_mlp_kernel<decltype(w)::value>), dim3((unsigned int)tiles), dim3(SA_THREADS), 0, (hipStream_t)stream, a);
    });
}
