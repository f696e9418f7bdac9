// PointNet++ set abstraction for inference, fused (include/pcr.h, pcr_pn2_sa_mlp_max): gather the ball's rows, run the shared MLP with
// the batch norm folded into its weights, ReLU, and keep the maximum over the ball -- the grouped tensor (b, C, m, nsample) never
// exists in memory.  Device pointers in, one kernel on the caller's stream, no context, no allocation, no wait.
//
// Arithmetic.  A gathered entry is xyz - new_xyz in binary32 (use_xyz), or the point's feature as stored.  The layers, their padding
// and why no stored bit depends on it are pcr_pn2_mlp_tile.h's (pn2_tile_layers); every layer here ends in its ReLU.
// A padded ROW (the last tile of a unit) gathers a copy of the unit's last real row, so it holds finite data, and the pooling loop
// runs over real rows only: it can never win a maximum.  A padded channel is never pooled.
//
// Tiling.  A workgroup of four waves owns a UNIT: G = 64 / nsample whole centres when nsample <= 64, one centre otherwise, and walks
// the unit's rows 64 at a time.  So no two workgroups ever share a centre: one plain store per (channel, centre), no atomics, no
// zeroing of `out`.  Per tile of 64 rows:
//   gather    row -> its point and its centre, once per tile in LDS (1 KiB); layer 0 reads its elements through them;
//   layers    pn2_tile_layers, which leaves the last activations in LDS (64 x width, row stride WMAX + 1);
//   pooling   one thread per (centre, channel) takes the maximum over the centre's rows of the tile; a centre of more than 64 rows
//             keeps its running maximum in the register of thread `channel` across its tiles.
// LDS and registers per variant: the shared header's budget plus the 1 KiB above, 33.75 / 58 / 106.5 KiB of the CU's 160.
#include "pcr_internal.h"
#include "pcr_pn2_mlp_tile.h"

namespace {

struct sa_args {
    int n, m, nsample, c_feat, use_xyz;
    int group;                         // centres per unit
    long long centres;                 // b * m
    long long out_batch_stride;
    pn2_layers layers;
    const float* xyz;
    const float* new_xyz;
    const float* feats;
    const int* idx;
    float* out;
};

template <int WMAX>
__global__ __launch_bounds__(SA_THREADS) void sa_mlp_max_kernel(const sa_args p) {
    constexpr int LDA = WMAX + 1;
    __shared__ float s_act[SA_TM * LDA];
    __shared__ float s_w[WMAX * SA_LDK];
    __shared__ float s_x[SA_TM * SA_LDK];
    __shared__ long long s_pt[SA_TM];                // row -> bi * n + point
    __shared__ long long s_cg[SA_TM];                // row -> bi * m + centre

    const int tid = threadIdx.x;
    const long long c0 = (long long)blockIdx.x * p.group;                                   // first centre of the unit
    const int gt = (int)(p.centres - c0 < p.group ? p.centres - c0 : (long long)p.group);   // its centres
    const int unit_rows = gt * p.nsample;
    const int c_last = p.layers.N[p.layers.n_layers - 1];
    const int xo = p.use_xyz ? 3 : 0;                // the relative coordinates come first
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

        // element k of row r: xyz - new_xyz, then the point's features
        pn2_tile_layers<WMAX>(p.layers, true, s_act, s_w, s_x, [&](int r, int k) {
            return k < xo ? p.xyz[s_pt[r] * 3 + k] - p.new_xyz[s_cg[r] * 3 + k] : p.feats[s_pt[r] * p.c_feat + (k - xo)];
        });

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

}  // namespace

extern "C" int pcr_pn2_sa_mlp_max(void* stream, int b, int n, int m, int nsample, int c_feat, int use_xyz, const float* xyz, const float* new_xyz,
                                  const float* feats, const int32_t* idx, int n_layers, const int* widths, const float* const* weights,
                                  const float* const* biases, float* out, long long out_batch_stride) {
    const bool empty = b == 0 || m == 0;
    // the sizes (K_0 = 3 + c_feat must fit an int); for a call that is not empty, every pointer the kernel would read or write
    const bool args_ok = b >= 0 && n >= 0 && m >= 0 && nsample >= 0 && c_feat >= 0 && c_feat <= 0x7FFFFFFF - 3 &&
                         (empty || (nsample >= 1 && n >= 1 && idx && out && (!use_xyz || (xyz && new_xyz)) && (c_feat == 0 || feats) && out_batch_stride >= 0));
    sa_args a;
    int wmax = 0;
    const int st = pn2_layers_from(args_ok, empty, (use_xyz ? 3LL : 0LL) + c_feat, n_layers, widths, weights, biases, &a.layers, &wmax);
    if (st != PCR_OK || empty) return st;
    a.n = n; a.m = m; a.nsample = nsample; a.c_feat = c_feat; a.use_xyz = use_xyz ? 1 : 0;
    a.group = nsample <= SA_TM ? SA_TM / nsample : 1;
    a.centres = (long long)b * m;
    a.out_batch_stride = out_batch_stride;
    a.xyz = xyz; a.new_xyz = new_xyz; a.feats = feats; a.idx = idx; a.out = out;
    const long long units = (a.centres + a.group - 1) / a.group;
    if (units > 0x7FFFFFFF) return PCR_E_UNSUPPORTED;
    return pn2_launch_for_width(wmax, [&](auto w) {
        hipLaunchKernelGGL((sa_mlp_max_kernel<decltype(w)::value>), dim3((unsigned int)units), dim3(SA_THREADS), 0, (hipStream_t)stream, a);
    });
}
