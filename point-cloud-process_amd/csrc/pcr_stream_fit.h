// Host scaffold of a streaming fit: passes over device-resident rows (the records of a cloud, the rows of a matrix), one block per
// tile of rows, whose last block advances a loop state on the device (device side: block_tile_load and block_slab_sums of pcr_wave.h).
// GMM, K-Means and the K-Means stage of spectral clustering are built on it; a new streaming feature starts here.
//
// Contract of a loop state: a plain struct whose first two ints are `it` (completed iterations) and `stop` (no further pass may run;
// passes enqueued behind a stop return at once), small enough for pcr_d2h_small.  Contract of a pass kernel: the parameters (rows, n,
// k, state, slabs, ticket, ...the pass's own); over a cloud it is a template on the dimension (2 or 3).
#pragma once
#include "pcr_internal.h"

struct pcr_stream_fit {
    pcr_ctx* ctx;
    const void* rows = nullptr;       // what the passes stream over
    long long n = 0;
    int k = 0, dim = 0;
    unsigned int grid = 0;            // blocks = tiles of the rows
    pcr_dev_block st;                 // the loop state
    unsigned int* ticket = nullptr;   // word of ctx->d_counters: zero between launches, re-armed by the last block
    explicit pcr_stream_fit(pcr_ctx* c) : ctx(c), st(c) {}
};

// state allocated and uploaded (stream-ordered: `h_state` must outlive the call that reads it back), slabs of `nsum_max` doubles per block
static inline int pcr_stream_begin(pcr_stream_fit* r, const void* rows, long long n, int k, int dim, int tile, pcr_cw ticket_user,
                                   const void* h_state, size_t state_bytes, int nsum_max) {
    pcr_ctx* ctx = r->ctx;
    r->rows = rows; r->n = n; r->k = k; r->dim = dim;
    r->grid = (unsigned int)((n + tile - 1) / tile);
    r->ticket = pcr_counter(ctx, ticket_user);
    int rc;
    if ((rc = r->st.alloc(state_bytes)) || (rc = pcr_ensure_scratch(ctx, sizeof(double) * nsum_max * (size_t)r->grid))) return rc;
    PCR_HIP(ctx, hipMemcpyAsync(r->st.p, h_state, state_bytes, hipMemcpyHostToDevice, ctx->stream));
    return PCR_OK;
}

// one pass: 256 threads per tile
template <class Row, class State, class... Params, class... Args>
static inline int pcr_stream_launch_one(const pcr_stream_fit* r, void (*kernel)(const Row*, long long, int, State*, double*, unsigned int*, Params...), Args... args) {
    pcr_ctx* ctx = r->ctx;
    hipLaunchKernelGGL(kernel, dim3(r->grid), dim3(256), 0, ctx->stream, (const Row*)r->rows, r->n, r->k, r->st.as<State>(), ctx->d_partials, r->ticket, (Params)args...);
    PCR_HIP(ctx, hipGetLastError());
    return PCR_OK;
}
// ... the <2> or <3> instantiation of a kernel by the fit's dimension
template <class Kernel, class... Args>
static inline int pcr_stream_launch(const pcr_stream_fit* r, Kernel k2, Kernel k3, Args... args) {
    return pcr_stream_launch_one(r, r->dim == 3 ? k3 : k2, args...);
}

// enqueue(i) enqueues the passes of iteration i < n_iter; after every `iters_per_sync` iterations and after the last one the first
// `head_bytes` of the state are read back, and the loop ends once `stop` is set
struct pcr_stream_head { int it, stop; };
template <class Enqueue>
static inline int pcr_stream_loop(pcr_stream_fit* r, int n_iter, int iters_per_sync, size_t head_bytes, Enqueue enqueue) {
    union { pcr_stream_head h; unsigned char bytes[256]; } head;
    if (head_bytes < sizeof(pcr_stream_head) || head_bytes > sizeof(head)) return PCR_E_INVALID;
    int rc;
    for (int i = 0; i < n_iter; ++i) {
        if ((rc = enqueue(i))) return rc;
        if (i + 1 == n_iter || (i + 1) % iters_per_sync == 0) {
            if ((rc = pcr_d2h_small(r->ctx, &head, r->st.p, head_bytes))) return rc;
            if (head.h.stop) break;
        }
    }
    return PCR_OK;
}

// milliseconds between ctx->ev0 and ctx->ev1, both recorded on the stream by the caller (waits for ev1)
static inline int pcr_events_ms(pcr_ctx* ctx, double* ms_out) {
    PCR_HIP(ctx, pcr_event_sync(ctx->ev1));
    float ms = 0;
    hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
    *ms_out = ms;
    return PCR_OK;
}
