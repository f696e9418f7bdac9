// PointNet++ gradients in a written order (include/pcr.h, "PointNet++ gradients"): the transposes of gather, group and
// three_interpolate.  Each is out[b, c, i] = sum of term[b, c, slot] over the slots with idx[b, slot] == i, added one by one in
// ASCENDING slot order onto +0.0f in binary32 (-ffp-contract=off), so np.add.at on a float32 array gives the same bits and two runs
// give the same bits.  No floating-point atomics (the only atomics are the integer ones inside the sort).
//
// Two steps.  (1) The inverse index of an index tensor, built once and shared by every channel (and by every tensor grouped with
// the same idx): start[b, 0..n] and slots[b, 0..k), point i's slots being slots[b, start[b,i] .. start[b,i+1]), ascending.  A stable
// radix sort of the pairs (b * n + idx[b, slot], slot) over the whole batch (pcr_sort.h) leaves exactly that in the values; start
// is a lower bound per point in the sorted keys.  The pairs are unique, so the result is a function of idx alone.  (2) The sum: every
// output is one strictly sequential chain of additions, so the parallelism is the number of chains.  A workgroup owns a cloud, a tile
// of PN2_GRAD_CT channels and a tile of up to PN2_GRAD_POINTS points, one thread per point with PN2_GRAD_CT accumulators in registers
// (that many independent chains in flight per thread, one read of the slot list for all of them).  It walks k in ascending chunks of
// PN2_GRAD_CHUNK slots: the chunk's terms go into LDS with coalesced reads (for the interpolation the product grad * weight is
// rounded there, once), then every thread advances its own list while its next slot lies inside the chunk.  Ascending chunks and
// ascending lists keep the order.  The lists are very uneven (ball query pads a short row with its first hit), which costs lanes
// that wait, never order.  A chunk in which no point of the tile has a slot is not staged.
#include <cstdint>
#include <cstring>
#include "pcr_sort.h"

namespace {

constexpr int PN2_GRAD_CT = 8;          // channels per workgroup = accumulators per thread
constexpr int PN2_GRAD_CHUNK = 1024;    // slots per LDS stage: 8 x 1024 floats = 32 KiB, four workgroups per CU
constexpr int PN2_GRAD_POINTS = 256;    // points (= threads) per workgroup; threads without a point still help to stage
constexpr int PN2_GRAD_AHEAD = 8;       // slot-list entries read per group; the next group is in flight while one is added
constexpr int PN2_INV_BLOCK = 256;

// ---------------------------------------------------------------- inverse index
__global__ __launch_bounds__(PN2_INV_BLOCK) void pn2_inv_keys_kernel(long long total, int n, int k, const int* __restrict__ idx,
                                                                     unsigned int* __restrict__ keys, int* __restrict__ vals) {
    for (long long g = (long long)blockIdx.x * PN2_INV_BLOCK + threadIdx.x; g < total; g += (long long)gridDim.x * PN2_INV_BLOCK) {
        const long long bi = g / k;
        keys[g] = (unsigned int)(bi * n + idx[g]);     // (b * n <= 2^32: checked by the entry)
        vals[g] = (int)(g - bi * k);
    }
}

// start[bi, i] = the number of cloud bi's sorted keys below bi * n + i; cloud bi's keys are sorted[bi * k .. (bi + 1) * k)
__global__ __launch_bounds__(PN2_INV_BLOCK) void pn2_inv_start_kernel(long long total, int n, int k, const unsigned int* __restrict__ sorted,
                                                                      int* __restrict__ start) {
    for (long long g = (long long)blockIdx.x * PN2_INV_BLOCK + threadIdx.x; g < total; g += (long long)gridDim.x * PN2_INV_BLOCK) {
        const long long bi = g / (n + 1);
        const int i = (int)(g - bi * (n + 1));
        int lo = 0, hi = k;
        if (i == n) lo = k;
        else {
            const unsigned int want = (unsigned int)(bi * n + i);
            const unsigned int* __restrict__ keys = sorted + bi * k;
            while (lo < hi) {
                const int mid = lo + ((hi - lo) >> 1);
                if (keys[mid] < want) lo = mid + 1;
                else hi = mid;
            }
        }
        start[g] = lo;
    }
}

static unsigned int pn2_inv_blocks(long long total) {
    const long long blocks = (total + PN2_INV_BLOCK - 1) / PN2_INV_BLOCK;
    return (unsigned int)(blocks < 65536 ? blocks : 65536);   // grid-stride beyond
}

static size_t pn2_align(size_t v) { return (v + 255) & ~(size_t)255; }

static unsigned int pn2_key_bits(long long keys) {   // bits that hold 0 .. keys - 1
    unsigned int bits = 1;
    while (bits < 32 && (1ll << bits) < keys) ++bits;
    return bits;
}

// workspace: keys in | keys sorted | values in | the sort's own temporary
static hipError_t pn2_inv_sort(void* temp, size_t& temp_bytes, unsigned int* keys_in, unsigned int* keys_out, int* vals_in, int* vals_out, size_t pairs,
                               unsigned int bits, hipStream_t s) {
    return pcr_sort_pairs(temp, temp_bytes, keys_in, keys_out, vals_in, vals_out, pairs, bits, s);
}

static int pn2_inv_check(int b, int n, int k) {
    if (b < 0 || n < 0 || k < 0) return PCR_E_INVALID;
    if ((long long)b * n > (1ll << 32)) return PCR_E_UNSUPPORTED;   // the sort's keys are 32 bits
    return PCR_OK;
}

// ---------------------------------------------------------------- the ordered sum
// WEIGHTED: term[c, slot] = grad[b, c, slot / 3] * weight[b, slot] (k = 3 * row_len); else term[c, slot] = grad[b, c, slot] (k = row_len)
template <bool WEIGHTED>
__global__ __launch_bounds__(PN2_GRAD_POINTS) void pn2_ordered_sum_kernel(int c, int n, int k, int row_len, const float* __restrict__ grad,
                                                                          const float* __restrict__ weight, const int* __restrict__ start_all,
                                                                          const int* __restrict__ slots_all, float* __restrict__ out) {
    // slot-major: row l holds the chunk's slot l for the tile's 8 channels as two float4 (one thread stages a row: coalesced reads
    // along the slots, 16-byte LDS writes 32 bytes apart, no bank conflict).  Row PN2_GRAD_CHUNK holds -0.0f, the one value x with
    // acc + x == acc for every acc, so a list entry outside the chunk is an addition that changes nothing, not a branch.
    __shared__ float4 s_term[2 * (PN2_GRAD_CHUNK + 1)];
    static_assert(PN2_GRAD_CT == 8, "a row of s_term is two float4");
    const int T = blockDim.x, tid = threadIdx.x;
    const int bi = blockIdx.z, c0 = blockIdx.y * PN2_GRAD_CT, i = blockIdx.x * T + tid;
    const int nc = min(PN2_GRAD_CT, c - c0);
    const int* __restrict__ slots = slots_all + (size_t)bi * k;
    const float* __restrict__ g = grad + ((size_t)bi * c + c0) * row_len;
    const float* __restrict__ w = WEIGHTED ? weight + (size_t)bi * k : nullptr;
    if (tid < 2) s_term[2 * PN2_GRAD_CHUNK + tid] = make_float4(-0.0f, -0.0f, -0.0f, -0.0f);   // (read behind the loop's barriers only)
    int p = 0, e = 0;
    if (i < n) {
        p = start_all[(size_t)bi * (n + 1) + i];
        e = start_all[(size_t)bi * (n + 1) + i + 1];
    }
    int next = p < e ? slots[p] : 0x7FFFFFFF;
    float acc[PN2_GRAD_CT];
#pragma unroll
    for (int q = 0; q < PN2_GRAD_CT; ++q) acc[q] = 0.0f;

    for (long long first = 0; first < k; first += PN2_GRAD_CHUNK) {   // (64 bits: k may lie within a chunk of 2^31 - 1)
        const int chunk0 = (int)first, len = min(PN2_GRAD_CHUNK, k - chunk0), chunk_end = chunk0 + len;
        // (the barrier in here also keeps the stage below from overwriting terms that a thread still reads)
        if (!__syncthreads_or(next < chunk_end)) continue;
        for (int l = tid; l < len; l += T) {
            const int slot = chunk0 + l;
            const size_t col = WEIGHTED ? slot / 3 : slot;
            const float wv = WEIGHTED ? w[slot] : 0.0f;
            float v[PN2_GRAD_CT];
#pragma unroll
            for (int q = 0; q < PN2_GRAD_CT; ++q) {
                v[q] = 0.0f;                                         // (channels behind nc: sums nobody stores)
                if (q < nc) v[q] = WEIGHTED ? g[(size_t)q * row_len + col] * wv : g[(size_t)q * row_len + col];
            }
            s_term[2 * l] = make_float4(v[0], v[1], v[2], v[3]);
            s_term[2 * l + 1] = make_float4(v[4], v[5], v[6], v[7]);
        }
        __syncthreads();
        if (next < chunk_end) {
            // the list entries come PN2_GRAD_AHEAD at a time and the next group's loads are issued before this group's additions; a
            // group is 2 * PN2_GRAD_AHEAD LDS reads in flight together, then its additions in list order.  A long list (one point
            // that most slots name) then costs a few instructions per term, not a memory or LDS round trip per term.
            int cur[PN2_GRAD_AHEAD], nxt[PN2_GRAD_AHEAD];
#pragma unroll
            for (int a = 0; a < PN2_GRAD_AHEAD; ++a) cur[a] = e - p > a ? slots[p + a] : 0x7FFFFFFF;
            for (;;) {
#pragma unroll
                for (int a = 0; a < PN2_GRAD_AHEAD; ++a) nxt[a] = e - p > PN2_GRAD_AHEAD + a ? slots[p + PN2_GRAD_AHEAD + a] : 0x7FFFFFFF;
                int used = 0;
                next = 0x7FFFFFFF;
#pragma unroll
                for (int a = PN2_GRAD_AHEAD - 1; a >= 0; --a)
                    if (cur[a] >= chunk_end) next = cur[a];          // ends as the first entry outside the chunk (ascending entries)
                float4 lo[PN2_GRAD_AHEAD], hi[PN2_GRAD_AHEAD];
#pragma unroll
                for (int a = 0; a < PN2_GRAD_AHEAD; ++a) {
                    const bool in = cur[a] < chunk_end;              // ascending: once one is outside, the rest are
                    const int l = in ? cur[a] - chunk0 : PN2_GRAD_CHUNK;
                    lo[a] = s_term[2 * l];
                    hi[a] = s_term[2 * l + 1];
                    used += in ? 1 : 0;
                }
#pragma unroll
                for (int a = 0; a < PN2_GRAD_AHEAD; ++a) {
                    acc[0] = acc[0] + lo[a].x; acc[1] = acc[1] + lo[a].y; acc[2] = acc[2] + lo[a].z; acc[3] = acc[3] + lo[a].w;
                    acc[4] = acc[4] + hi[a].x; acc[5] = acc[5] + hi[a].y; acc[6] = acc[6] + hi[a].z; acc[7] = acc[7] + hi[a].w;
                }
                p += used;
                if (used < PN2_GRAD_AHEAD) break;                    // the chunk's last entry of this list, or the list's
#pragma unroll
                for (int a = 0; a < PN2_GRAD_AHEAD; ++a) cur[a] = nxt[a];
            }
        }
    }
    if (i < n)
        for (int q = 0; q < nc; ++q) out[((size_t)bi * c + c0 + q) * n + i] = acc[q];
}

// b, c, n, k > 0 here
template <bool WEIGHTED>
static int pn2_ordered_sum(hipStream_t s, int b, int c, int n, int k, int row_len, const float* grad, const float* weight, const int* start, const int* slots,
                           float* out) {
    const int threads = PN2_GRAD_POINTS;
    const int point_tiles = (n + threads - 1) / threads, channel_tiles = (c + PN2_GRAD_CT - 1) / PN2_GRAD_CT;
    if (channel_tiles > 65535 || b > 65535) return PCR_E_UNSUPPORTED;   // grid y and z
    hipLaunchKernelGGL((pn2_ordered_sum_kernel<WEIGHTED>), dim3((unsigned int)point_tiles, (unsigned int)channel_tiles, (unsigned int)b), dim3((unsigned int)threads),
                       0, s, c, n, k, row_len, grad, weight, start, slots, out);
    return hipGetLastError() == hipSuccess ? PCR_OK : PCR_E_HIP;
}

// the three entries behind their own argument checks; k == 0 with a non-empty output: zeros
static int pn2_grad_entry(void* stream, int b, int c, int n, long long k, int row_len, const float* grad, const float* weight, const int* start,
                          const int* slots, float* out) {
    if (b == 0 || c == 0 || n == 0) return PCR_OK;
    if (k > 0x7FFFFFFFll) return PCR_E_UNSUPPORTED;
    if (!out) return PCR_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    if (k == 0) return hipMemsetAsync(out, 0, (size_t)b * c * n * sizeof(float), s) == hipSuccess ? PCR_OK : PCR_E_HIP;
    if (!grad || !start || !slots) return PCR_E_INVALID;
    if (weight) return pn2_ordered_sum<true>(s, b, c, n, (int)k, row_len, grad, weight, start, slots, out);
    return pn2_ordered_sum<false>(s, b, c, n, (int)k, row_len, grad, nullptr, start, slots, out);
}

}  // namespace

extern "C" {

long long pcr_pn2_inverse_index_bytes(int b, int n, int k) {
    const int rc = pn2_inv_check(b, n, k);
    if (rc) return rc;
    const size_t pairs = (size_t)b * k;
    if (pairs == 0) return 0;
    size_t temp_bytes = 0;
    if (pn2_inv_sort(nullptr, temp_bytes, nullptr, nullptr, nullptr, nullptr, pairs, pn2_key_bits((long long)b * n), nullptr) != hipSuccess) return PCR_E_HIP;
    return (long long)(3 * pn2_align(pairs * 4) + pn2_align(temp_bytes));
}

int pcr_pn2_inverse_index(void* stream, int b, int n, int k, const int32_t* idx, void* workspace, long long workspace_bytes, int32_t* start_out,
                          int32_t* slots_out) {
    const int rc = pn2_inv_check(b, n, k);
    if (rc) return rc;
    if (b == 0) return PCR_OK;
    if (!start_out) return PCR_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const long long starts = (long long)b * (n + 1ll);
    if (k == 0) return hipMemsetAsync(start_out, 0, (size_t)starts * sizeof(int32_t), s) == hipSuccess ? PCR_OK : PCR_E_HIP;
    if (n == 0 || !idx || !slots_out || !workspace || ((uintptr_t)workspace & 255)) return PCR_E_INVALID;
    const size_t pairs = (size_t)b * k, part = pn2_align(pairs * 4);
    const unsigned int bits = pn2_key_bits((long long)b * n);
    size_t temp_bytes = 0;
    if (pn2_inv_sort(nullptr, temp_bytes, nullptr, nullptr, nullptr, nullptr, pairs, bits, s) != hipSuccess) return PCR_E_HIP;
    if (workspace_bytes < 0 || (size_t)workspace_bytes < 3 * part + pn2_align(temp_bytes)) return PCR_E_INVALID;
    char* ws = (char*)workspace;
    unsigned int* keys_in = (unsigned int*)ws;
    unsigned int* keys_out = (unsigned int*)(ws + part);
    int* vals_in = (int*)(ws + 2 * part);
    hipLaunchKernelGGL(pn2_inv_keys_kernel, dim3(pn2_inv_blocks((long long)pairs)), dim3(PN2_INV_BLOCK), 0, s, (long long)pairs, n, k, idx, keys_in, vals_in);
    if (hipGetLastError() != hipSuccess) return PCR_E_HIP;
    if (pn2_inv_sort(ws + 3 * part, temp_bytes, keys_in, keys_out, vals_in, slots_out, pairs, bits, s) != hipSuccess) return PCR_E_HIP;
    hipLaunchKernelGGL(pn2_inv_start_kernel, dim3(pn2_inv_blocks(starts)), dim3(PN2_INV_BLOCK), 0, s, starts, n, k, keys_out, start_out);
    return hipGetLastError() == hipSuccess ? PCR_OK : PCR_E_HIP;
}

int pcr_pn2_gather_points_grad(void* stream, int b, int c, int n, int npoints, const float* grad_out, const int32_t* start, const int32_t* slots,
                               float* grad_points) {
    if (b < 0 || c < 0 || n < 0 || npoints < 0) return PCR_E_INVALID;
    return pn2_grad_entry(stream, b, c, n, npoints, npoints, grad_out, nullptr, start, slots, grad_points);
}

int pcr_pn2_group_points_grad(void* stream, int b, int c, int n, int npoints, int nsample, const float* grad_out, const int32_t* start, const int32_t* slots,
                              float* grad_points) {
    if (b < 0 || c < 0 || n < 0 || npoints < 0 || nsample < 0) return PCR_E_INVALID;
    const long long k = (long long)npoints * nsample;
    return pn2_grad_entry(stream, b, c, n, k, (int)(k > 0x7FFFFFFFll ? 0 : k), grad_out, nullptr, start, slots, grad_points);
}

int pcr_pn2_three_interpolate_grad(void* stream, int b, int c, int n, int m, const float* grad_out, const int32_t* start, const int32_t* slots,
                                   const float* weight, float* grad_points) {
    if (b < 0 || c < 0 || n < 0 || m < 0) return PCR_E_INVALID;
    if (b && c && m && n && !weight) return PCR_E_INVALID;
    return pn2_grad_entry(stream, b, c, m, 3ll * n, n, grad_out, weight, start, slots, grad_points);
}

}  // extern "C"
