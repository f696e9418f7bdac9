// (key, value) sorts of the set-up paths: rocPRIM's radix sort with the merge-sort cross-over moved.  Its default configuration
// merge-sorts up to ~1 M pairs; measured on MI355X (scripts/sort_bench.hip, 30-bit keys, us): 120 000 pairs merge 48-58 /
// onesweep 103-118; 1 M pairs merge 160-190 / onesweep 103-134; 10 M pairs 400-550 either way.  So: merge sort below 400 000
// pairs, onesweep above.
#pragma once
#include <rocprim/rocprim.hpp>
#include "pcr_internal.h"

using pcr_sort_config = rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config, rocprim::default_config, 400000>;

template <typename K, typename V>
static inline hipError_t pcr_sort_pairs(void* temp, size_t& temp_bytes, K* keys_in, K* keys_out, V* vals_in, V* vals_out, size_t n, unsigned int end_bit,
                                        hipStream_t stream) {
    return rocprim::radix_sort_pairs<pcr_sort_config>(temp, temp_bytes, keys_in, keys_out, vals_in, vals_out, n, 0u, end_bit, stream);
}

// the sort as its callers use it: the temporary's size asked for, the temporary taken from the arena (`temp` owns it: the caller
// keeps it alive until the stream has passed the sort, i.e. to the end of its own scope), the sort enqueued
template <typename K, typename V>
static inline int pcr_sort_pairs_arena(pcr_ctx* ctx, K* keys_in, K* keys_out, V* vals_in, V* vals_out, size_t n, unsigned int end_bit, pcr_dev_block& temp) {
    size_t temp_bytes = 0;
    int rc;
    PCR_HIP(ctx, pcr_sort_pairs(nullptr, temp_bytes, keys_in, keys_out, vals_in, vals_out, n, end_bit, ctx->stream));
    if ((rc = temp.alloc(temp_bytes))) return rc;
    PCR_HIP(ctx, pcr_sort_pairs(temp.p, temp_bytes, keys_in, keys_out, vals_in, vals_out, n, end_bit, ctx->stream));
    return PCR_OK;
}

// the positions 0 .. n - 1 whose flag is set, ascending -> out[0 .. *d_count) (rocprim::select over a counting iterator): the
// temporary's size asked for, the temporary taken from the arena (`temp` owns it, as above), the select enqueued.  `flags`: any iterator
// (an array on the device, or a transform iterator that computes the flag); Out: the integer type of the positions.  `who`: the caller's
// name for the text of a HIP error ("who (select): ...").
template <typename Flags, typename Out>
static inline int pcr_select_positions(pcr_ctx* ctx, Flags flags, size_t n, Out* out, unsigned int* d_count, pcr_dev_block& temp, const char* who = nullptr) {
    const auto positions = rocprim::counting_iterator<Out>(0);
    size_t temp_bytes = 0;
    int rc = PCR_OK;
    hipError_t e = rocprim::select(nullptr, temp_bytes, positions, flags, out, d_count, n, ctx->stream);
    if (e == hipSuccess && (rc = temp.alloc(temp_bytes)) == PCR_OK) e = rocprim::select(temp.p, temp_bytes, positions, flags, out, d_count, n, ctx->stream);
    if (rc) return rc;
    if (e != hipSuccess) {
        ctx->last_error = (who ? std::string(who) + " (select): " : std::string("rocprim::select: ")) + hipGetErrorString(e);
        return PCR_E_HIP;
    }
    return PCR_OK;
}

template <typename K>
struct head_flag {  // position i starts a group of equal keys
    const K* keys;
    __host__ __device__ bool operator()(unsigned int i) const { return i == 0u || keys[i] != keys[i - 1u]; }
};

// group heads of n sorted keys = positions whose key differs from the previous one -> heads[0 .. *n_groups): one fused flag + scan +
// scatter (the select with a computed flag), instead of a flag kernel, a scan and a scatter
template <typename K>
static inline int pcr_group_heads(pcr_ctx* ctx, const K* sorted_keys, size_t n, unsigned int* heads, unsigned int* n_groups, pcr_dev_block& temp) {
    const auto flags = rocprim::make_transform_iterator(rocprim::counting_iterator<unsigned int>(0u), head_flag<K>{sorted_keys});
    return pcr_select_positions(ctx, flags, n, heads, n_groups, temp);
}
