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

template <typename K>
struct head_flag {  // position i starts a group of equal keys
    const K* keys;
    __host__ __device__ bool operator()(unsigned int i) const { return i == 0u || keys[i] != keys[i - 1u]; }
};

// group heads of n sorted keys = positions whose key differs from the previous one -> heads[0 .. *n_groups): one fused flag + scan +
// scatter (rocprim::select over a counting iterator with a computed flag), instead of a flag kernel, a scan and a scatter
template <typename K>
static inline int pcr_group_heads(pcr_ctx* ctx, const K* sorted_keys, size_t n, unsigned int* heads, unsigned int* n_groups, pcr_dev_block& temp) {
    const head_flag<K> flag_op{sorted_keys};
    auto positions = rocprim::counting_iterator<unsigned int>(0u);
    auto flags = rocprim::make_transform_iterator(positions, flag_op);
    size_t temp_bytes = 0;
    int rc;
    PCR_HIP(ctx, rocprim::select(nullptr, temp_bytes, positions, flags, heads, n_groups, n, ctx->stream));
    if ((rc = temp.alloc(temp_bytes))) return rc;
    PCR_HIP(ctx, rocprim::select(temp.p, temp_bytes, positions, flags, heads, n_groups, n, ctx->stream));
    return PCR_OK;
}
