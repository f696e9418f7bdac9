// pcr_debug_linalg: the small dense solves of pcr_linalg.h, one problem per device lane (ctx) or in a host loop (ctx == NULL).
// Diagnostics only: the hot paths call these functions from the finishing lane of their own kernels (pcr_icp_step.h, pcr_harris.hip,
// pcr_shot.hip, pcr_point2plane.hip); this entry point lets tests hand the DEVICE build of each function its edge inputs directly
// (tests/linalg_checks.py).  Every lane copies its inputs into locals, calls exactly the pcr:: function and writes its outputs; the
// unit is compiled with the library's flags, so contraction is what the header's own pragmas ask for.
#include "pcr_internal.h"
#include "pcr_linalg.h"

namespace {

constexpr int LP_OPS = 6;
constexpr int LP_MAX_N = 65536;
// doubles per problem (include/pcr.h lists what they are)
constexpr int lp_in(int op) { return op == 0 ? 9 : op == 1 ? 18 : op == 2 ? 6 : op == 3 ? 21 : op == 4 ? 30 : 27; }
constexpr int lp_out(int op) { return op == 0 ? 21 : op == 1 ? 21 : op == 2 ? 18 : op == 3 ? 13 : op == 4 ? 22 : 23; }

template <int OP>
__host__ __device__ inline void lp_solve(const double* in, double* out) {
    if constexpr (OP == 0 || OP == 1) {          // svd3, cold / warm: H[9] (, V0[9]) -> U[9], s[3], V[9]
        double H[9], V0[9], U[9], s[3], V[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) { H[i] = in[i]; V0[i] = OP == 1 ? in[9 + i] : 0.0; U[i] = NAN; V[i] = NAN; }   // (an element svd3 left unwritten would show)
        s[0] = s[1] = s[2] = NAN;
        pcr::svd3(H, U, s, V, OP == 1 ? V0 : nullptr);
#pragma unroll
        for (int i = 0; i < 9; ++i) { out[i] = U[i]; out[12 + i] = V[i]; }
#pragma unroll
        for (int i = 0; i < 3; ++i) out[9 + i] = s[i];
    } else if constexpr (OP == 2) {              // sym3_jacobi: upper triangle (00 01 02 11 12 22) -> A after [9], Q[9]
        double A[3][3] = {{in[0], in[1], in[2]}, {in[1], in[3], in[4]}, {in[2], in[4], in[5]}};
        double Q[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
        pcr::sym3_jacobi(A, Q);
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) { out[3 * i + j] = A[i][j]; out[9 + 3 * i + j] = Q[i][j]; }
    } else if constexpr (OP == 3 || OP == 4) {   // kabsch_from_moments: m[18], origin[3] (, V[9]) -> R[9], t[3], cost (, V[9])
        double m[18], origin[3], V[9], R[9], t[3], cost = NAN;
#pragma unroll
        for (int i = 0; i < 18; ++i) m[i] = in[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) { origin[i] = in[18 + i]; t[i] = NAN; }
#pragma unroll
        for (int i = 0; i < 9; ++i) { V[i] = OP == 4 ? in[21 + i] : 0.0; R[i] = NAN; }
        pcr::kabsch_from_moments(m, origin, R, t, &cost, OP == 4 ? V : nullptr);
#pragma unroll
        for (int i = 0; i < 9; ++i) out[i] = R[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) out[9 + i] = t[i];
        out[12] = cost;
        if constexpr (OP == 4) {
#pragma unroll
            for (int i = 0; i < 9; ++i) out[13 + i] = V[i];
        }
    } else {                                     // point2plane_solve: Au[21], b[6] -> x[6], U[16], ok
        double Au[21], b[6], x[6], U[16];
#pragma unroll
        for (int i = 0; i < 21; ++i) Au[i] = in[i];
#pragma unroll
        for (int i = 0; i < 6; ++i) { b[i] = in[21 + i]; x[i] = NAN; }
#pragma unroll
        for (int i = 0; i < 16; ++i) U[i] = NAN;
        const bool ok = pcr::point2plane_solve(Au, b, x, U);
#pragma unroll
        for (int i = 0; i < 6; ++i) out[i] = x[i];
#pragma unroll
        for (int i = 0; i < 16; ++i) out[6 + i] = U[i];
        out[22] = ok ? 1.0 : 0.0;
    }
}

// one problem per lane, blocks of one wave; lanes past n do nothing
template <int OP>
__global__ __launch_bounds__(64) void linalg_probe_kernel(const double* __restrict__ in, long long n, double* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    lp_solve<OP>(in + i * lp_in(OP), out + i * lp_out(OP));
}

template <int OP>
void lp_host(const double* in, int64_t n, double* out) {
    for (int64_t i = 0; i < n; ++i) lp_solve<OP>(in + i * lp_in(OP), out + i * lp_out(OP));
}

template <int OP>
void lp_launch(pcr_ctx* ctx, const double* d_in, int64_t n, double* d_out) {
    hipLaunchKernelGGL(linalg_probe_kernel<OP>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, ctx->stream, d_in, (long long)n, d_out);
}

}  // namespace

extern "C" {

int pcr_debug_linalg(pcr_ctx* ctx, int op, const double* in, int64_t n, double* out) try {
    if (op < 0 || op >= LP_OPS || !in || !out || n < 0 || n > LP_MAX_N) return PCR_E_INVALID;
    if (n == 0) return PCR_OK;
    if (!ctx) {   // the host build of the same functions
        switch (op) {
            case 0: lp_host<0>(in, n, out); break;
            case 1: lp_host<1>(in, n, out); break;
            case 2: lp_host<2>(in, n, out); break;
            case 3: lp_host<3>(in, n, out); break;
            case 4: lp_host<4>(in, n, out); break;
            default: lp_host<5>(in, n, out); break;
        }
        return PCR_OK;
    }
    hipSetDevice(ctx->device);
    pcr_dev_block d_in(ctx), d_out(ctx);   // (back to the arena on every return path)
    int rc;
    if ((rc = d_in.alloc(sizeof(double) * lp_in(op) * (size_t)n)) || (rc = d_out.alloc(sizeof(double) * lp_out(op) * (size_t)n))) return rc;
    PCR_HIP(ctx, hipMemcpyAsync(d_in.p, in, sizeof(double) * lp_in(op) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    switch (op) {
        case 0: lp_launch<0>(ctx, d_in.as<const double>(), n, d_out.as<double>()); break;
        case 1: lp_launch<1>(ctx, d_in.as<const double>(), n, d_out.as<double>()); break;
        case 2: lp_launch<2>(ctx, d_in.as<const double>(), n, d_out.as<double>()); break;
        case 3: lp_launch<3>(ctx, d_in.as<const double>(), n, d_out.as<double>()); break;
        case 4: lp_launch<4>(ctx, d_in.as<const double>(), n, d_out.as<double>()); break;
        default: lp_launch<5>(ctx, d_in.as<const double>(), n, d_out.as<double>()); break;
    }
    PCR_HIP(ctx, hipGetLastError());
    PCR_HIP(ctx, hipMemcpyAsync(out, d_out.p, sizeof(double) * lp_out(op) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    PCR_HIP(ctx, pcr_sync(ctx->stream));
    return PCR_OK;
} PCR_CATCH(ctx)

}  // extern "C"
