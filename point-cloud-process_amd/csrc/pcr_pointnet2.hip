// PointNet++ set-abstraction ops on the caller's device tensors (include/pcr.h, "PointNet++ set-abstraction ops"): furthest point
// sampling, ball query, three_nn, three_interpolate, gather, group.  Device pointers in, kernels enqueued on the caller's stream, no
// context, no allocation, no wait.  Everything is binary32 in the written order (-ffp-contract=off), so tests/pointnet2_checks.py
// reproduces every output bit for bit.
#include "pcr_wave.h"

namespace {

__device__ static inline float pn2_d2(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return ((dx * dx) + (dy * dy)) + (dz * dz);
}

// ---------------------------------------------------------------- furthest point sampling
// One workgroup per cloud; the picks are a serial chain, so a pick must be short: thread t owns points t, t + T, t + 2T, ... and keeps
// the first Q of them (coordinates and running distance) in registers, the next PN2_FPS_LDS_POINTS of the block in LDS, and only what
// is left (n > Q*T + PN2_FPS_LDS_POINTS) in memory, with its running distances in `temp`.  A point that is not eligible has the
// running distance -1, which min(d, -1) keeps without a test.  Per pick a thread updates its points and keeps the largest running
// distance and the lowest of its points that has it (one block of CU arithmetic does all of a cloud's points, so the instructions per
// point ARE the pick time at large n: 8 for the distance, 1 minimum, 1 compare, 2 selects), then packs them into
// key = (bits(temp) ^ sign) << 32 | ~k: floats >= 0 order like their bits and -1 falls below them, so ONE unsigned maximum is "largest
// distance, lowest index among equals, eligible before not".  The wave reduces the key on the DPP network, the lane that owns the
// wave's maximum (keys carry k: exactly one) writes the key and its point's coordinates into the wave's slot, ONE barrier, then
// every wave reduces the slots for itself and reads the winner's coordinates from its slot.  The slots are double-buffered: a wave
// that writes slot row j & 1 for pick j + 2 has passed the barrier of pick j + 1, which every wave reaches only after it has read
// that row for pick j.  A winning key without the top bit: nothing is eligible, the pick is index 0.
constexpr int PN2_FPS_MAX_THREADS = 1024;
constexpr int PN2_FPS_MAX_Q = 16;               // points per thread in registers (124 of the 128 VGPRs a 1 024-thread block may have): n <= 16 384
constexpr int PN2_FPS_LDS_POINTS = 8192;        // 16 B each: 128 KiB of the CU's 160
constexpr float PN2_FPS_FAR = 1e10f;

struct __attribute__((aligned(32))) pn2_fps_slot {
    unsigned long long key;
    float x, y, z, pad;
};

__device__ static inline float pn2_fps_temp0(float x, float y, float z) {
    const float mag = ((x * x) + (y * y)) + (z * z);
    return (double)mag <= 1e-3 ? -1.0f : PN2_FPS_FAR;
}

template <int Q, int LDS_POINTS>
__global__ __launch_bounds__(PN2_FPS_MAX_THREADS) void pn2_fps_kernel(int n, int m, const float* __restrict__ xyz_all, float* __restrict__ temp_all,
                                                                        int* __restrict__ idx_all) {
    __shared__ pn2_fps_slot s_slot[2][16];
    __shared__ float4 s_pts[LDS_POINTS ? LDS_POINTS : 1];
    const int T = blockDim.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = T >> 6;
    const float* __restrict__ xyz = xyz_all + (size_t)blockIdx.x * n * 3;
    float* __restrict__ temp = temp_all + (size_t)blockIdx.x * n;
    int* __restrict__ idx = idx_all + (size_t)blockIdx.x * m;
    const int reg_end = Q * T;                                          // (Q * T <= 16 384)
    const int lds_end = LDS_POINTS ? min(n, reg_end + LDS_POINTS) : reg_end;

    float rx[Q], ry[Q], rz[Q], rt[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int k = q * T + tid, kc = min(k, n - 1);   // (no branch: a slot behind the end reads the last point and is not eligible)
        rx[q] = xyz[3 * (size_t)kc]; ry[q] = xyz[3 * (size_t)kc + 1]; rz[q] = xyz[3 * (size_t)kc + 2];
        const float t0 = pn2_fps_temp0(rx[q], ry[q], rz[q]);
        rt[q] = k < n ? t0 : -1.0f;
    }
    if (LDS_POINTS) {   // a thread only ever touches its own LDS and `temp` entries: no barrier behind the fill
        for (int k = reg_end + tid; k < lds_end; k += T) {
            const float x = xyz[3 * (size_t)k], y = xyz[3 * (size_t)k + 1], z = xyz[3 * (size_t)k + 2];
            s_pts[k - reg_end] = make_float4(x, y, z, pn2_fps_temp0(x, y, z));
        }
        for (int k = lds_end + tid; k < n; k += T) temp[k] = pn2_fps_temp0(xyz[3 * (size_t)k], xyz[3 * (size_t)k + 1], xyz[3 * (size_t)k + 2]);
    }
    float cx = xyz[0], cy = xyz[1], cz = xyz[2];
    if (tid == 0) idx[0] = 0;

    for (int j = 1; j < m; ++j) {
        // registers from the last point down with >=, so that the lowest of equals stays; the tiers behind have higher numbers: >
        float bt = -1.0f;
        int bq = 0;
#pragma unroll
        for (int q = Q - 1; q >= 0; --q) {
            rt[q] = fminf(pn2_d2(rx[q], ry[q], rz[q], cx, cy, cz), rt[q]);
            if (rt[q] >= bt) { bt = rt[q]; bq = q; }
        }
        int bk = bq * T + tid;
        if (LDS_POINTS) {
            for (int k = reg_end + tid; k < lds_end; k += T) {
                const float4 p = s_pts[k - reg_end];
                const float t = fminf(pn2_d2(p.x, p.y, p.z, cx, cy, cz), p.w);
                s_pts[k - reg_end].w = t;
                if (t > bt) { bt = t; bk = k; }
            }
            for (int k = lds_end + tid; k < n; k += T) {
                float t = temp[k];
                if (t < 0.0f) continue;
                t = fminf(pn2_d2(xyz[3 * (size_t)k], xyz[3 * (size_t)k + 1], xyz[3 * (size_t)k + 2], cx, cy, cz), t);
                temp[k] = t;
                if (t > bt) { bt = t; bk = k; }
            }
        }
        const unsigned long long best = ((unsigned long long)(__float_as_uint(bt) ^ 0x80000000u) << 32) | (0xFFFFFFFFu - (unsigned int)bk);
        const unsigned long long wmax = wave_max_u64(best);
        pn2_fps_slot* row = s_slot[j & 1];
        if (best == wmax) {   // one lane: bk differs from lane to lane
            float x = rx[0], y = ry[0], z = rz[0];
#pragma unroll
            for (int q = 1; q < Q; ++q)
                if (bq == q) { x = rx[q]; y = ry[q]; z = rz[q]; }
            if (LDS_POINTS && bk >= reg_end) {
                if (bk < lds_end) { const float4 p = s_pts[bk - reg_end]; x = p.x; y = p.y; z = p.z; }
                else { x = xyz[3 * (size_t)bk]; y = xyz[3 * (size_t)bk + 1]; z = xyz[3 * (size_t)bk + 2]; }
            }
            row[wave].key = wmax;
            row[wave].x = x; row[wave].y = y; row[wave].z = z;
        }
        __syncthreads();
        const unsigned long long mine = (lane & 15) < nwaves ? row[lane & 15].key : 0ull;
        const unsigned long long rmax = row_max_u64(mine);   // every row of 16 lanes holds the same 16 slots
        const unsigned long long gmax = ((unsigned long long)(unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)(rmax >> 32), 15) << 32) |
                                        (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)rmax, 15);
        const int w = (__ffsll((long long)__ballot(mine == gmax)) - 1) & 15;   // (every key is > 0, the filler of the unused slots)
        cx = row[w].x; cy = row[w].y; cz = row[w].z;
        if (tid == 0) idx[j] = (gmax >> 63) ? (int)(0xFFFFFFFFu - (unsigned int)gmax) : 0;
    }
}

template <int Q, int LDS_POINTS>
static hipError_t pn2_fps_launch(hipStream_t s, int b, int n, int m, int threads, const float* xyz, float* temp, int* idx) {
    hipLaunchKernelGGL((pn2_fps_kernel<Q, LDS_POINTS>), dim3((unsigned int)b), dim3((unsigned int)threads), 0, s, n, m, xyz, temp, idx);
    return hipGetLastError();
}

// ---------------------------------------------------------------- ball query
// 16 waves per block, one centre per wave; the block walks the cloud through LDS tiles (every tile is read from memory once per 16
// centres).  A wave tests 64 consecutive points per step: the ballot of the hits and each hit's rank below its lane (mbcnt) give its
// output slot, so a row comes out in index order without any sorting; a wave with nsample hits is done, and the block leaves the
// cloud as soon as all its waves are.
constexpr int PN2_BQ_WAVES = 16;
constexpr int PN2_BQ_TILE = 4096;   // points per LDS tile (48 KiB as three planes)

__global__ __launch_bounds__(PN2_BQ_WAVES * 64) void pn2_ball_query_kernel(int n, int m, float r2, int nsample, const float* __restrict__ new_xyz_all,
                                                                            const float* __restrict__ xyz_all, int* __restrict__ idx_all) {
    __shared__ float s_x[PN2_BQ_TILE], s_y[PN2_BQ_TILE], s_z[PN2_BQ_TILE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int per_cloud = (m + PN2_BQ_WAVES - 1) / PN2_BQ_WAVES;   // blocks
    const int bi = blockIdx.x / per_cloud, centre = (blockIdx.x - bi * per_cloud) * PN2_BQ_WAVES + wave;
    const bool active = centre < m;
    const float* __restrict__ xyz = xyz_all + (size_t)bi * n * 3;
    float qx = 0.0f, qy = 0.0f, qz = 0.0f;
    int* __restrict__ out = idx_all;
    if (active) {
        const float* q = new_xyz_all + ((size_t)bi * m + centre) * 3;
        qx = q[0]; qy = q[1]; qz = q[2];
        out = idx_all + ((size_t)bi * m + centre) * nsample;
    }
    int cnt = 0, first = 0;
    bool done = !active;
    for (int base = 0; base < n; base += PN2_BQ_TILE) {
        const int tn = min(PN2_BQ_TILE, n - base);
        for (int i = tid; i < 3 * tn; i += PN2_BQ_WAVES * 64) {
            const float v = xyz[3 * (size_t)base + i];
            const int p = i / 3, c = i - 3 * p;
            (c == 0 ? s_x : c == 1 ? s_y : s_z)[p] = v;
        }
        __syncthreads();
        if (!done) {
            for (int c0 = 0; c0 < tn; c0 += 64) {   // (wave-uniform loop: cnt, first and done are the same in all lanes)
                const int p = c0 + lane;
                const bool hit = p < tn && pn2_d2(qx, qy, qz, s_x[p < tn ? p : 0], s_y[p < tn ? p : 0], s_z[p < tn ? p : 0]) < r2;
                const unsigned long long mask = __ballot(hit);
                if (!mask) continue;
                const int slot = cnt + (int)__builtin_amdgcn_mbcnt_hi((unsigned int)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)mask, 0u));
                if (hit && slot < nsample) out[slot] = base + p;
                if (cnt == 0) first = base + c0 + __ffsll((long long)mask) - 1;
                cnt += __popcll(mask);
                if (cnt >= nsample) { done = true; break; }
            }
        }
        if (__syncthreads_and(done)) break;   // (also: nobody still reads the tile that the next round overwrites)
    }
    if (active)
        for (int sl = cnt + lane; sl < nsample; sl += 64) out[sl] = first;   // fewer hits than slots: the first hit; none: 0
}

// ---------------------------------------------------------------- three_nn
// One thread per unknown point, the known points through LDS tiles that the whole block reads at the same address (a broadcast).
constexpr int PN2_NN_BLOCK = 256;
constexpr int PN2_NN_TILE = 2048;

__global__ __launch_bounds__(PN2_NN_BLOCK) void pn2_three_nn_kernel(int n, int m, const float* __restrict__ unknown_all, const float* __restrict__ known_all,
                                                                    float* __restrict__ dist2_all, int* __restrict__ idx_all) {
    __shared__ float s_k[3 * PN2_NN_TILE];
    const int per_cloud = (n + PN2_NN_BLOCK - 1) / PN2_NN_BLOCK;   // blocks
    const int bi = blockIdx.x / per_cloud, i = (blockIdx.x - bi * per_cloud) * PN2_NN_BLOCK + threadIdx.x;
    const float* __restrict__ known = known_all + (size_t)bi * m * 3;
    float ux = 0.0f, uy = 0.0f, uz = 0.0f;
    if (i < n) {
        const float* u = unknown_all + ((size_t)bi * n + i) * 3;
        ux = u[0]; uy = u[1]; uz = u[2];
    }
    float b1 = __builtin_inff(), b2 = __builtin_inff(), b3 = __builtin_inff();
    int i1 = 0, i2 = 0, i3 = 0;
    for (int base = 0; base < m; base += PN2_NN_TILE) {
        const int tn = min(PN2_NN_TILE, m - base);
        if (base) __syncthreads();
        for (int t = threadIdx.x; t < 3 * tn; t += PN2_NN_BLOCK) s_k[t] = known[3 * (size_t)base + t];
        __syncthreads();
        for (int k = 0; k < tn; ++k) {
            const float d = pn2_d2(ux, uy, uz, s_k[3 * k], s_k[3 * k + 1], s_k[3 * k + 2]);
            if (d < b1) { b3 = b2; i3 = i2; b2 = b1; i2 = i1; b1 = d; i1 = base + k; }
            else if (d < b2) { b3 = b2; i3 = i2; b2 = d; i2 = base + k; }
            else if (d < b3) { b3 = d; i3 = base + k; }
        }
    }
    if (i < n) {
        float* dout = dist2_all + ((size_t)bi * n + i) * 3;
        int* io = idx_all + ((size_t)bi * n + i) * 3;
        dout[0] = b1; dout[1] = b2; dout[2] = b3;
        io[0] = i1; io[1] = i2; io[2] = i3;
    }
}

// ---------------------------------------------------------------- interpolate, gather, group: one thread per output element
constexpr int PN2_EW_BLOCK = 256;

__global__ __launch_bounds__(PN2_EW_BLOCK) void pn2_three_interpolate_kernel(long long total, int c, int m, int n, const float* __restrict__ points,
                                                                             const int* __restrict__ idx, const float* __restrict__ weight, float* __restrict__ out) {
    for (long long e = (long long)blockIdx.x * PN2_EW_BLOCK + threadIdx.x; e < total; e += (long long)gridDim.x * PN2_EW_BLOCK) {
        const long long row = e / n;                 // b * c + channel
        const int i = (int)(e - row * n);
        const long long bi = row / c;
        const int* id = idx + (bi * n + i) * 3;
        const float* w = weight + (bi * n + i) * 3;
        const float* p = points + row * m;
        out[e] = ((p[id[0]] * w[0]) + (p[id[1]] * w[1])) + (p[id[2]] * w[2]);
    }
}

// out[row, j] = points[row, idx[row / c, j]]: gather (per = npoints) and group (per = npoints * nsample) are the same copy
__global__ __launch_bounds__(PN2_EW_BLOCK) void pn2_gather_kernel(long long total, int c, int n, long long per, const float* __restrict__ points,
                                                                  const int* __restrict__ idx, float* __restrict__ out) {
    for (long long e = (long long)blockIdx.x * PN2_EW_BLOCK + threadIdx.x; e < total; e += (long long)gridDim.x * PN2_EW_BLOCK) {
        const long long row = e / per, j = e - row * per;
        out[e] = points[row * n + idx[(row / c) * per + j]];
    }
}

static unsigned int pn2_ew_blocks(long long total) {
    const long long blocks = (total + PN2_EW_BLOCK - 1) / PN2_EW_BLOCK;
    return (unsigned int)(blocks < 65536 ? blocks : 65536);   // grid-stride beyond
}

static int pn2_gather(hipStream_t s, long long rows, int c, int n, long long per, const float* points, const int* idx, float* out) {
    const long long total = rows * per;
    hipLaunchKernelGGL(pn2_gather_kernel, dim3(pn2_ew_blocks(total)), dim3(PN2_EW_BLOCK), 0, s, total, c, n, per, points, idx, out);
    return hipGetLastError() == hipSuccess ? PCR_OK : PCR_E_HIP;
}

}  // namespace

extern "C" {

int pcr_pn2_furthest_point_sampling(void* stream, int b, int n, int m, const float* xyz, float* temp, int32_t* idx_out) {
    if (b < 0 || n < 0 || m < 0) return PCR_E_INVALID;
    if (b == 0 || m == 0) return PCR_OK;
    if (n == 0 || !xyz || !temp || !idx_out) return PCR_E_INVALID;
    // about four points per thread while the block grows, then more per thread; registers first, LDS and memory behind them
    int threads = ((n + 3) / 4 + 63) / 64 * 64;
    threads = threads < 64 ? 64 : threads > PN2_FPS_MAX_THREADS ? PN2_FPS_MAX_THREADS : threads;
    const int per = (n + threads - 1) / threads;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e;
    if (per <= 1) e = pn2_fps_launch<1, 0>(s, b, n, m, threads, xyz, temp, idx_out);
    else if (per <= 2) e = pn2_fps_launch<2, 0>(s, b, n, m, threads, xyz, temp, idx_out);
    else if (per <= 4) e = pn2_fps_launch<4, 0>(s, b, n, m, threads, xyz, temp, idx_out);
    else if (per <= 8) e = pn2_fps_launch<8, 0>(s, b, n, m, threads, xyz, temp, idx_out);
    else if (per <= PN2_FPS_MAX_Q) e = pn2_fps_launch<PN2_FPS_MAX_Q, 0>(s, b, n, m, threads, xyz, temp, idx_out);
    else e = pn2_fps_launch<PN2_FPS_MAX_Q, PN2_FPS_LDS_POINTS>(s, b, n, m, threads, xyz, temp, idx_out);
    return e == hipSuccess ? PCR_OK : PCR_E_HIP;
}

int pcr_pn2_ball_query(void* stream, int b, int n, int m, float radius, int nsample, const float* new_xyz, const float* xyz, int32_t* idx_out) {
    if (b < 0 || n < 0 || m < 0 || nsample < 0) return PCR_E_INVALID;
    if (b == 0 || m == 0 || nsample == 0) return PCR_OK;
    const long long blocks = (long long)b * ((m + PN2_BQ_WAVES - 1) / PN2_BQ_WAVES);
    if (n == 0 || !(radius - radius == 0.0f) || !new_xyz || !xyz || !idx_out || blocks > 0x7FFFFFFF) return PCR_E_INVALID;
    const float r2 = radius * radius;
    hipLaunchKernelGGL(pn2_ball_query_kernel, dim3((unsigned int)blocks), dim3(PN2_BQ_WAVES * 64), 0,
                       (hipStream_t)stream, n, m, r2, nsample, new_xyz, xyz, idx_out);
    return hipGetLastError() == hipSuccess ? PCR_OK : PCR_E_HIP;
}

int pcr_pn2_three_nn(void* stream, int b, int n, int m, const float* unknown, const float* known, float* dist2_out, int32_t* idx_out) {
    if (b < 0 || n < 0 || m < 0) return PCR_E_INVALID;
    if (b == 0 || n == 0) return PCR_OK;
    const long long blocks = (long long)b * ((n + PN2_NN_BLOCK - 1) / PN2_NN_BLOCK);
    if (m == 0 || !unknown || !known || !dist2_out || !idx_out || blocks > 0x7FFFFFFF) return PCR_E_INVALID;
    hipLaunchKernelGGL(pn2_three_nn_kernel, dim3((unsigned int)blocks), dim3(PN2_NN_BLOCK), 0,
                       (hipStream_t)stream, n, m, unknown, known, dist2_out, idx_out);
    return hipGetLastError() == hipSuccess ? PCR_OK : PCR_E_HIP;
}

int pcr_pn2_three_interpolate(void* stream, int b, int c, int m, int n, const float* points, const int32_t* idx, const float* weight, float* out) {
    if (b < 0 || c < 0 || m < 0 || n < 0) return PCR_E_INVALID;
    if (b == 0 || c == 0 || n == 0) return PCR_OK;
    if (m == 0 || !points || !idx || !weight || !out) return PCR_E_INVALID;
    const long long total = (long long)b * c * n;
    hipLaunchKernelGGL(pn2_three_interpolate_kernel, dim3(pn2_ew_blocks(total)), dim3(PN2_EW_BLOCK), 0, (hipStream_t)stream, total, c, m, n, points, idx, weight, out);
    return hipGetLastError() == hipSuccess ? PCR_OK : PCR_E_HIP;
}

int pcr_pn2_gather_points(void* stream, int b, int c, int n, int npoints, const float* points, const int32_t* idx, float* out) {
    if (b < 0 || c < 0 || n < 0 || npoints < 0) return PCR_E_INVALID;
    if (b == 0 || c == 0 || npoints == 0) return PCR_OK;
    if (n == 0 || !points || !idx || !out) return PCR_E_INVALID;
    return pn2_gather((hipStream_t)stream, (long long)b * c, c, n, npoints, points, idx, out);
}

int pcr_pn2_group_points(void* stream, int b, int c, int n, int npoints, int nsample, const float* points, const int32_t* idx, float* out) {
    if (b < 0 || c < 0 || n < 0 || npoints < 0 || nsample < 0) return PCR_E_INVALID;
    if (b == 0 || c == 0 || npoints == 0 || nsample == 0) return PCR_OK;
    if (n == 0 || !points || !idx || !out) return PCR_E_INVALID;
    return pn2_gather((hipStream_t)stream, (long long)b * c, c, n, (long long)npoints * nsample, points, idx, out);
}

}  // extern "C"
