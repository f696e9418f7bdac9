// One pass of Lloyd's iteration over a source of rows, instantiated by pcr_kmeans.hip for the 32-byte records of a
// cloud and by pcr_spectral.hip for the rows of an embedding.
//   lloyd_assign   label = argmin_k d2 under the CURRENT centres (direct form, lowest k on ties), per cluster the exact count N_k and
//                  S_k = sum x, and the inertia of the current centres.  The block that takes the last ticket divides, keeps the centre
//                  of an empty cluster, applies the stop rule and writes the next centres;
//   lloyd_label    the final pass and predict: labels, counts and inertia under the given centres.
// Centres are broadcast from LDS.  A lane keeps its rows and their labels in registers; clusters go by in chunks whose masked
// accumulators (label == k ? x : 0) stay in registers, so the order of every sum is fixed: per lane over its rows in order (from 0.0
// where it has several, the value itself where it has one), wave totals on the DPP network, then block_slab_sums.  Counts are integers
// all the way.  No floating-point atomics, the block count depends on n alone: two runs give the same bits.
// A source `Src` names: rec (what the first kernel parameter points to), KMAX, CSTRIDE (doubles per centre in the state), PTS (rows
// per lane), DMAX (coordinates a row is unrolled to), CHUNK (clusters per chunk), NSUM (doubles per slab, >= KMAX (1 + DMAX) + 1),
// dims(m) (the coordinates in use: a constant, or m <= DMAX at run time) and load(rows, n, m, x, valid, row): this block's tile, zeros
// and valid = false behind the end, row = where the label goes.
#pragma once
#include <cstddef>
#include "pcr_internal.h"
#include "pcr_wave.h"

// Loop state on the device: the first 40 bytes are the head the host reads per chunk of iterations; a user derives to append fields.
template <int KMAX, int CSTRIDE>
struct __attribute__((aligned(16))) lloyd_state {
    int it;              // completed iterations
    int stop;            // no further assign pass may run
    int converged;       // stopped by shift <= tol
    int n_empty;         // clusters without points in the last pass that counted
    int max_iter, pad;
    double inertia;      // of the centres the last pass assigned under
    double shift;        // max_k |c_new[k] - c_old[k]| of the last update
    double tol;
    double c[KMAX * CSTRIDE];      // current centres
    long long counts[KMAX];        // N_k of the last pass
};
constexpr size_t LLOYD_HEAD_BYTES = 40;
constexpr int LLOYD_ITERS_PER_SYNC = 8;   // iterations enqueued per read-back of the loop state's head
using lloyd_state_1 = lloyd_state<1, 1>;
static_assert(offsetof(lloyd_state_1, tol) == LLOYD_HEAD_BYTES, "head of the loop state");

template <class Src>
struct lloyd_lds {
    double part[4][Src::NSUM], red[8][Src::NSUM], tot[Src::NSUM];
    double c[Src::KMAX * Src::CSTRIDE];
};

// block_slab_sums (pcr_wave.h) with integer adds in the count slots (t < K * nt with t % nt == 0), binary64 adds elsewhere
struct lloyd_slot_add {
    int K, nt;
    __device__ double operator()(double x, double y, int t) const {
        const bool count = t < K * nt && t % nt == 0;
        return count ? __longlong_as_double(__double_as_longlong(x) + __double_as_longlong(y)) : x + y;
    }
};

// squared distance in the direct form, the order of np.sum over (dx^2, dy^2, ...)
template <class Src>
__device__ inline double lloyd_d2(const double* c, const double (&x)[Src::DMAX], int dims) {
    const double d0 = x[0] - c[0];
    double d2 = d0 * d0;
#pragma unroll
    for (int d = 1; d < Src::DMAX; ++d)
        if (d < dims) { const double dd = x[d] - c[d]; d2 = d2 + dd * dd; }
    return d2;
}

// The block's tile under the centres of `st`: labels (if asked for), and per wave in s.part the cluster values (SUMS: N_k, S_k at
// [k * (1 + dims), ...); else N_k at [k]) and the inertia behind them; then the slabs.  True in the block that arrived last: s.tot
// holds the totals.
template <class Src, bool SUMS>
__device__ inline bool lloyd_block_pass(const typename Src::rec* __restrict__ rows, long long n, int m, int K,
                                        const lloyd_state<Src::KMAX, Src::CSTRIDE>* __restrict__ st, int* __restrict__ labels, double* __restrict__ partials,
                                        unsigned int* __restrict__ ticket, lloyd_lds<Src>& s) {
    constexpr int PTS = Src::PTS, DMAX = Src::DMAX, CHUNK = Src::CHUNK;
    const int dims = Src::dims(m), nt = SUMS ? 1 + dims : 1;
    for (int t = threadIdx.x; t < K * Src::CSTRIDE; t += PCR_STREAM_BLOCK) s.c[t] = st->c[t];
    double x[PTS][DMAX];
    int lab[PTS];
    long long row[PTS];
    bool valid[PTS];
    Src::load(rows, n, m, x, valid, row);
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double inertia = 0.0;
#pragma unroll
    for (int p = 0; p < PTS; ++p) {
        double best = lloyd_d2<Src>(s.c, x[p], dims);
        int arg = 0;
#pragma unroll 4   // (left to itself the compiler may take 8 on the cloud source: the registers drop <3> from 7 waves per SIMD to 4)
        for (int k = 1; k < K; ++k) {
            const double d = lloyd_d2<Src>(s.c + Src::CSTRIDE * k, x[p], dims);
            if (d < best) { best = d; arg = k; }
        }
        lab[p] = valid[p] ? arg : -1;
        const double v = valid[p] ? best : 0.0;
        inertia = PTS == 1 ? v : inertia + v;
        if (valid[p] && labels) labels[row[p]] = arg;
    }
    inertia = wave_total_f64(inertia);
    if (lane == 63) s.part[wave][K * nt] = inertia;
    for (int k0 = 0; k0 < K; k0 += CHUNK) {
        double acc[CHUNK][DMAX] = {};
        unsigned int cnt[CHUNK] = {};
#pragma unroll
        for (int p = 0; p < PTS; ++p) {
#pragma unroll
            for (int j = 0; j < CHUNK; ++j) {
                const bool mine = lab[p] == k0 + j;
                cnt[j] += mine ? 1u : 0u;
                if (SUMS) {
#pragma unroll
                    for (int d = 0; d < DMAX; ++d) {
                        const double v = mine ? x[p][d] : 0.0;
                        acc[j][d] = PTS == 1 ? v : acc[j][d] + v;
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < CHUNK; ++j) {
            const unsigned int c = wave_incl_scan_add(cnt[j]);   // total in lane 63; every lane takes part
            if (lane == 63 && k0 + j < K) s.part[wave][(k0 + j) * nt] = __longlong_as_double((long long)c);
            if (SUMS) {
#pragma unroll
                for (int d = 0; d < DMAX; ++d) {
                    if (d < dims) {   // (uniform)
                        const double v = wave_total_f64(acc[j][d]);
                        if (lane == 63 && k0 + j < K) s.part[wave][(k0 + j) * nt + 1 + d] = v;
                    }
                }
            }
        }
    }
    return block_slab_sums<Src::NSUM>(s.part, K * nt + 1, partials, ticket, s.red, s.tot, lloyd_slot_add{K, nt});
}

// One Lloyd iteration.  Slab layout: cluster k at [k * (1 + dims), ...) = N_k (integer), S_k; the inertia at K * (1 + dims).  True
// in every thread of the block that arrived last: s.tot still holds the totals.  Its thread 0 calls done(it, inertia, shift) with the
// index of the iteration it has just completed.
template <class Src, class Done>
__device__ inline bool lloyd_assign(const typename Src::rec* __restrict__ rows, long long n, int m, int K, lloyd_state<Src::KMAX, Src::CSTRIDE>* __restrict__ st,
                                    double* __restrict__ partials, unsigned int* __restrict__ ticket, lloyd_lds<Src>& s, Done done) {
    if (st->stop) return false;
    if (!lloyd_block_pass<Src, true>(rows, n, m, K, st, nullptr, partials, ticket, s)) return false;

    // ---- the last block: the new centres (an empty cluster keeps its own), the shift, the stop rule
    const int dims = Src::dims(m), nt = 1 + dims;
    double *s_shift = s.red[0], *s_count = s.red[1];   // (the slices are spent)
    const int k = threadIdx.x;
    if (k < K) {
        const long long nk = __double_as_longlong(s.tot[k * nt]);
        double q = 0.0;
#pragma unroll
        for (int d = 0; d < Src::DMAX; ++d) {
            if (d < dims) {
                const double old = s.c[Src::CSTRIDE * k + d];
                const double cn = nk > 0 ? s.tot[k * nt + 1 + d] / (double)nk : old;
                const double dd = cn - old;
                q = d == 0 ? dd * dd : q + dd * dd;
                st->c[Src::CSTRIDE * k + d] = cn;
            }
        }
        s_shift[k] = sqrt(q);
        s_count[k] = s.tot[k * nt];
        st->counts[k] = nk;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double shift = 0.0;
        int n_empty = 0;
        for (int j = 0; j < K; ++j) {
            shift = s_shift[j] > shift ? s_shift[j] : shift;
            n_empty += __double_as_longlong(s_count[j]) > 0 ? 0 : 1;
        }
        const int it = st->it;
        const double inertia = s.tot[K * nt];
        done(it, inertia, shift);
        st->inertia = inertia;
        st->shift = shift;
        st->n_empty = n_empty;
        st->it = it + 1;
        if (shift <= st->tol) { st->converged = 1; st->stop = 1; }
        else if (it + 1 >= st->max_iter) st->stop = 1;
    }
    return true;
}

// The final pass and predict: labels (or none), the counts and the inertia under the centres of `st`.  Slab layout: N_k at [k], the
// inertia at [K].
template <class Src>
__device__ inline void lloyd_label(const typename Src::rec* __restrict__ rows, long long n, int m, int K, lloyd_state<Src::KMAX, Src::CSTRIDE>* __restrict__ st,
                                   double* __restrict__ partials, unsigned int* __restrict__ ticket, int* __restrict__ labels, lloyd_lds<Src>& s) {
    if (!lloyd_block_pass<Src, false>(rows, n, m, K, st, labels, partials, ticket, s) || threadIdx.x != 0) return;
    int n_empty = 0;
    for (int j = 0; j < K; ++j) {
        const long long nk = __double_as_longlong(s.tot[j]);
        st->counts[j] = nk;
        n_empty += nk > 0 ? 0 : 1;
    }
    st->n_empty = n_empty;
    st->inertia = s.tot[K];
}
