// Wave64 primitives, the per-block tile load and the slab reduction of the streaming passes: nothing here knows about the grid.
#pragma once
#include "pcr_internal.h"

// ---------------------------------------------------------------- wave64 reductions on the DPP network
// row_shr 1 / 2 / 4 / 8, then row_bcast15 / row_bcast31: six VALU instructions of a few cycles each, no LDS traffic (a __shfl_up / __shfl_xor
// chain is six DEPENDENT ds_bpermute round trips).  All 64 lanes must be active.
template <int CTRL, int ROW_MASK>
__device__ static inline unsigned int dpp_u32(unsigned int identity, unsigned int v) {
    return (unsigned int)__builtin_amdgcn_update_dpp((int)identity, (int)v, CTRL, ROW_MASK, 0xf, false);
}
__device__ static inline unsigned int wave_incl_scan_add(unsigned int v) {
    v += dpp_u32<0x111, 0xf>(0u, v);
    v += dpp_u32<0x112, 0xf>(0u, v);
    v += dpp_u32<0x114, 0xf>(0u, v);
    v += dpp_u32<0x118, 0xf>(0u, v);
    v += dpp_u32<0x142, 0xa>(0u, v);   // row_bcast15 into rows 1 and 3
    v += dpp_u32<0x143, 0xc>(0u, v);   // row_bcast31 into rows 2 and 3
    return v;
}
__device__ static inline unsigned int wave_excl_scan_u32(unsigned int v, int lane, unsigned int* total) {
    const unsigned int inc = wave_incl_scan_add(v);
    *total = __builtin_amdgcn_readlane((int)inc, 63);
    return inc - v;
}
// binary64 wave total in lane 63 (inclusive-scan pattern; lanes without a source add +0.0)
template <int CTRL, int ROW_MASK>
__device__ static inline double dpp_add_f64(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROW_MASK, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROW_MASK, 0xf, false);
    return v + __hiloint2double(hi, lo);
}
__device__ static inline double wave_total_f64(double v) {
    v = dpp_add_f64<0x111, 0xf>(v);
    v = dpp_add_f64<0x112, 0xf>(v);
    v = dpp_add_f64<0x114, 0xf>(v);
    v = dpp_add_f64<0x118, 0xf>(v);
    v = dpp_add_f64<0x142, 0xa>(v);
    v = dpp_add_f64<0x143, 0xc>(v);
    return v;
}
// minimum / maximum over the wave in every lane (lanes without a source keep their own value; lane 63 ends with the result)
__device__ static inline int wave_min_i32(int v) {
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x111, 0xf, 0xf, false));
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x112, 0xf, 0xf, false));
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x114, 0xf, 0xf, false));
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x118, 0xf, 0xf, false));
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x142, 0xa, 0xf, false));
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x143, 0xc, 0xf, false));
    return __builtin_amdgcn_readlane(v, 63);
}
__device__ static inline int wave_max_i32(int v) {
    v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x111, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x112, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x114, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x118, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x142, 0xa, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x143, 0xc, 0xf, false));
    return __builtin_amdgcn_readlane(v, 63);
}
// unsigned 64-bit maximum on the same network (lanes without a source keep their own value).  row_max_u64: the first four steps, the
// maximum of each row of 16 lanes in its lane 15; wave_max_u64: the maximum of the wave, in every lane
template <int CTRL, int ROW_MASK>
__device__ static inline unsigned long long dpp_max_u64(unsigned long long v) {
    const unsigned int lo = (unsigned int)__builtin_amdgcn_update_dpp((int)(unsigned int)v, (int)(unsigned int)v, CTRL, ROW_MASK, 0xf, false);
    const unsigned int hi = (unsigned int)__builtin_amdgcn_update_dpp((int)(unsigned int)(v >> 32), (int)(unsigned int)(v >> 32), CTRL, ROW_MASK, 0xf, false);
    const unsigned long long o = ((unsigned long long)hi << 32) | lo;
    return o > v ? o : v;
}
__device__ static inline unsigned long long row_max_u64(unsigned long long v) {
    v = dpp_max_u64<0x111, 0xf>(v);
    v = dpp_max_u64<0x112, 0xf>(v);
    v = dpp_max_u64<0x114, 0xf>(v);
    v = dpp_max_u64<0x118, 0xf>(v);
    return v;
}
__device__ static inline unsigned long long wave_max_u64(unsigned long long v) {
    v = row_max_u64(v);
    v = dpp_max_u64<0x142, 0xa>(v);
    v = dpp_max_u64<0x143, 0xc>(v);
    return ((unsigned long long)(unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)(v >> 32), 63) << 32) | (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)v, 63);
}
__device__ static inline double vmin(double a, double b) {  // plain v_min_f64 (fmin() adds two canonicalising v_max)
    double r;
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// binary64 minimum over the wave in every lane: ~20 instructions of a few cycles each -- the __shfl_xor butterfly was six DEPENDENT
// ds_bpermute round trips (~0.3 us) in the middle of every step of a descent.  Lanes without a source keep their own value (old = self).
template <int CTRL, int ROW_MASK>
__device__ static inline double dpp_min_f64(double v) {
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(v), __double2loint(v), CTRL, ROW_MASK, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(v), __double2hiint(v), CTRL, ROW_MASK, 0xf, false);
    return vmin(v, __hiloint2double(hi, lo));
}
__device__ static inline double wave_min_f64(double v) {
    v = dpp_min_f64<0x111, 0xf>(v);
    v = dpp_min_f64<0x112, 0xf>(v);
    v = dpp_min_f64<0x114, 0xf>(v);
    v = dpp_min_f64<0x118, 0xf>(v);
    v = dpp_min_f64<0x142, 0xa>(v);
    v = dpp_min_f64<0x143, 0xc>(v);
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63), __builtin_amdgcn_readlane(__double2loint(v), 63));
}
__device__ static inline long long readlane_i64(long long v, int l) {   // l: wave-uniform
    return ((long long)__builtin_amdgcn_readlane((int)(v >> 32), l) << 32) | (unsigned int)__builtin_amdgcn_readlane((int)v, l);
}
__device__ static inline double readlane_f64(double v, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

// The tree of the object sum of include/pcr.h ("KITTI boxes", "label match"): lane l holds the sum of its rows l, l + 64, ...;
// p_l += p_{l+s} for l < s, s = 32 .. 1; p_0 to every lane.  (A lane >= s adds something it never hands on: at step s only lanes
// below 2s are read.)  All 64 lanes must be active.
__device__ static inline double wave_object_sum_f64(double p) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) p += __shfl_down(p, s, 64);
    return readlane_f64(p, 0);
}

// Wave sum by the xor butterfly, lane pairs 32 apart, then 16 .. 1: every lane ends with the same bits.  (Not wave_total_f64: that adds
// in another order and leaves the total in lane 63; the results that go through here are pinned to this order.)  All 64 lanes active.
__device__ static inline double wave_sum_all(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ static inline int wave_sum_all(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ static inline bool finite3(double x, double y, double z) { return x - x == 0.0 && y - y == 0.0 && z - z == 0.0; }

// LDS hand-off between the lanes of ONE wave: LDS operations of a wave execute in order, so no hardware wait is
// needed, but the compiler must neither forward a lane's own earlier store to its load nor move accesses across
__device__ static inline void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---------------------------------------------------------------- streaming passes: blocks of 256 threads = four waves
constexpr int PCR_STREAM_BLOCK = 256;

// This block's tile of PTS * 256 records, PTS per lane (point p of a lane is record (blockIdx.x * PTS + p) * 256 + threadIdx.x, so a
// wave reads 2 KiB in a row); behind the end: zeros, valid = false and id = -1.  ID = false: the pass does not use the caller rows,
// `id` may be null and costs no registers.
template <int PTS, bool ID>
__device__ static inline void block_tile_load(const pcr_pt* __restrict__ pts, long long n, double (&x)[PTS], double (&y)[PTS], double (&z)[PTS],
                                              bool (&valid)[PTS], long long* id) {
#pragma unroll
    for (int p = 0; p < PTS; ++p) {
        const long long i = ((long long)blockIdx.x * PTS + p) * PCR_STREAM_BLOCK + threadIdx.x;
        valid[p] = i < n;
        x[p] = y[p] = z[p] = 0.0;
        if (ID) id[p] = -1;
        if (valid[p]) { const pcr_pt r = pts[i]; x[p] = r.x; y[p] = r.y; z[p] = r.z; if (ID) id[p] = r.id; }
    }
}

// Block slabs with a last-block ticket.
// Block total of the per-wave values in s_part -> this block's slab of `nsum` values in `partials`; the block that arrives last adds
// the slabs in a fixed order into s_tot and gets true.  add(a, b, t) combines two values of slot t (a plain + for a double; an integer
// slot keeps its bits in the double).  The hand-off of grid_accumulate_kernel (pcr_grid_search.hip, which keeps its own copy): drained
// stores -> barrier -> agent-scope release -> ticket; last arriver: agent-scope acquire -> barrier -> plain loads.  The ticket word
// is re-armed for the next launch.
template <int NSUM_MAX, class Add>
__device__ static inline bool block_slab_sums(const double (*s_part)[NSUM_MAX], int nsum, double* __restrict__ partials, unsigned int* __restrict__ ticket,
                                              double (*s_red)[NSUM_MAX], double* s_tot, Add add) {
    __shared__ unsigned int s_last;
    __syncthreads();
    if ((int)threadIdx.x < nsum) {
        const int t = threadIdx.x;
        partials[(long long)blockIdx.x * nsum + t] = add(add(s_part[0][t], s_part[1][t], t), add(s_part[2][t], s_part[3][t], t), t);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned int t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = (t == gridDim.x - 1) ? 1u : 0u;
        if (s_last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            *ticket = 0;   // ready for the next launch (stream-ordered)
        }
    }
    __syncthreads();
    if (!s_last) return false;
    // 8 strided slices of the slabs (slice j: blocks j, j + 8, ... in order), then a fixed tree over the slices
    for (int idx = threadIdx.x; idx < 8 * nsum; idx += (int)blockDim.x) {
        const int slice = idx / nsum, t = idx - slice * nsum;
        double v = 0.0;   // all bits zero: the integer 0 as well
        for (long long b = slice; b < (long long)gridDim.x; b += 8) v = add(v, partials[b * nsum + t], t);
        s_red[slice][t] = v;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < nsum; t += (int)blockDim.x)
        s_tot[t] = add(add(add(s_red[0][t], s_red[1][t], t), add(s_red[2][t], s_red[3][t], t), t),
                       add(add(s_red[4][t], s_red[5][t], t), add(s_red[6][t], s_red[7][t], t), t), t);
    __syncthreads();
    return true;
}
