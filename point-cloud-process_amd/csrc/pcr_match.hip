// Feature matching of the global initialisation (stages: pcr_global_dev.h):
//   pcr_feature_match    nearest neighbour in feature space (find_matchings / the matching inside
//                        registration_ransac_based_on_feature_matching)   Registration/main.py:73, icp_template.py:20-41
// and the correspondence set RANSAC samples from.  A pair alone takes the plain kernel; the fused initialisation matches every
// pair of a share in one launch on the f64 matrix cores (operands prepared per chunk of scans), exactly.
#include <cfloat>
#include <cmath>
#include <cstring>
#include "pcr_grid_dev.h"
#include "pcr_linalg.h"
#include "pcr_global_dev.h"

// ----------------------------------------------------------- feature matching
// One thread per query row, target rows staged through LDS in tiles; squared L2 summed over the
// dimensions in order; ties to the lowest target row.
constexpr int FM_TILE = 32;
// grid = (query blocks, target splits): block (bx, by) scans targets [by * per, (by + 1) * per); a small merge kernel
// takes the minimum over the splits (ascending split order + strict comparison keeps the lowest row on ties).
template <int DIM>
__device__ static void feature_match_body(const double* __restrict__ A, long long na, const double* __restrict__ B, long long nb, int dim_rt, long long per,
                                          int* __restrict__ idx_out, double* __restrict__ d2_out, const unsigned int bx, const unsigned int by, double* tile /* LDS: FM_TILE * dim */) {
    const int dim = DIM > 0 ? DIM : dim_rt;
    const long long i = (long long)bx * blockDim.x + threadIdx.x;
    const bool live = i < na;
    double a[DIM > 0 ? DIM : 1];
    if (DIM > 0 && live) {
#pragma unroll
        for (int k = 0; k < DIM; ++k) a[k] = A[i * DIM + k];
    }
    double best = DBL_MAX;
    int bidx = -1;
    const long long tb = (long long)by * per, te = (tb + per < nb) ? tb + per : nb;
    for (long long t0 = tb; t0 < te; t0 += FM_TILE) {
        const int rows = (int)((te - t0) < FM_TILE ? (te - t0) : FM_TILE);
        __syncthreads();
        for (int e = threadIdx.x; e < rows * dim; e += blockDim.x) tile[e] = B[t0 * dim + e];
        __syncthreads();
        if (!live) continue;
        for (int r = 0; r < rows; ++r) {
            double s = 0.0;
            if (DIM > 0) {
#pragma unroll
                for (int k = 0; k < DIM; ++k) { const double d = a[k] - tile[r * DIM + k]; s += d * d; }
            } else {
                for (int k = 0; k < dim; ++k) { const double d = A[i * dim + k] - tile[r * dim + k]; s += d * d; }
            }
            if (s < best) { best = s; bidx = (int)(t0 + r); }
        }
    }
    if (live) { idx_out[(long long)by * na + i] = bidx; d2_out[(long long)by * na + i] = best; }
}
template <int DIM>
__global__ void __launch_bounds__(256) feature_match_kernel(const double* __restrict__ A, long long na, const double* __restrict__ B, long long nb, int dim_rt,
                                                             long long per, int* __restrict__ idx_out, double* __restrict__ d2_out) {
    extern __shared__ double tile[];  // FM_TILE * dim
    feature_match_body<DIM>(A, na, B, nb, dim_rt, per, idx_out, d2_out, blockIdx.x, blockIdx.y, tile);
}

__device__ static void feature_match_merge_body(const int* __restrict__ cidx, const double* __restrict__ cd2, long long na, int splits, int* __restrict__ idx_out,
                                                double* __restrict__ d2_out, const unsigned int bx) {
    const long long i = (long long)bx * blockDim.x + threadIdx.x;
    if (i >= na) return;
    double best = DBL_MAX;
    int bidx = -1;
    for (int sp = 0; sp < splits; ++sp) {
        const double d = cd2[(long long)sp * na + i];
        const int j = cidx[(long long)sp * na + i];
        if (j >= 0 && d < best) { best = d; bidx = j; }
    }
    idx_out[i] = bidx;
    d2_out[i] = best;
}
__global__ void feature_match_merge_kernel(const int* __restrict__ cidx, const double* __restrict__ cd2, long long na, int splits,
                                           int* __restrict__ idx_out, double* __restrict__ d2_out) {
    feature_match_merge_body(cidx, cd2, na, splits, idx_out, d2_out, blockIdx.x);
}

// correspondence set of registration_ransac_based_on_feature_matching: (i, ij[i]) for every source row, kept when mutual
// (ji[ij[i]] == i); when fewer than `min_mutual` survive, Open3D falls back to the one-way set.  ONE block, rows in order.
struct corr_lds { int w[4], total, use; };
__device__ static void corr_build_body(const int* __restrict__ ij, const int* __restrict__ ji, int na, int mutual, int min_mutual, int* __restrict__ corr,
                                       int* __restrict__ m_out, corr_lds* L) {
    int* const s_w = L->w;
    int& s_total = L->total;
    int& s_use = L->use;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_total = 0;
    __syncthreads();
    int mine = 0;
    if (mutual)
        for (int i = threadIdx.x; i < na; i += 256) mine += (ij[i] >= 0 && ji[ij[i]] == i) ? 1 : 0;
    if (mutual) atomicAdd(&s_total, mine);
    __syncthreads();
    if (threadIdx.x == 0) s_use = (mutual && s_total >= min_mutual) ? 1 : 0;
    __syncthreads();
    const int use_mutual = s_use;
    int base = 0;
    for (int i0 = 0; i0 < na; i0 += 256) {
        const int i = i0 + threadIdx.x;
        const bool keep = i < na && ij[i] >= 0 && (!use_mutual || ji[ij[i]] == i);
        const unsigned long long mk = __ballot(keep);
        if (lane == 0) s_w[wave] = __popcll(mk);
        __syncthreads();
        int off = base;
        for (int w = 0; w < wave; ++w) off += s_w[w];
        if (keep) {
            const int r = off + __popcll(mk & ((1ull << lane) - 1ull));
            corr[2 * r] = i;
            corr[2 * r + 1] = ij[i];
        }
        base += s_w[0] + s_w[1] + s_w[2] + s_w[3];
        __syncthreads();
    }
    if (threadIdx.x == 0) *m_out = base;
}
__global__ void __launch_bounds__(256) corr_build_kernel(const int* __restrict__ ij, const int* __restrict__ ji, int na, int mutual, int min_mutual,
                                                         int* __restrict__ corr, int* __restrict__ m_out) {
    __shared__ corr_lds s_L;
    corr_build_body(ij, ji, na, mutual, min_mutual, corr, m_out, &s_L);
}

// ---- feature matching on the matrix cores, exact.
// |a - b|^2 = |a|^2 + (|b|^2 - 2 a.b): the bracket is a K = 36 contraction [-2 b_0 .. -2 b_32, |b|^2, 0, 0] . [a_0 .. a_32, 1, 0, 0] -- nine
// v_mfma_f64_16x16x4_f64 per 16 targets x 16 queries -- and |a|^2 does not move a query's argmin.  The sweep is only a FILTER: per query and
// lane the running minimum m of the bracket and the targets within tau of it are kept (the true winner is within tau of the running minimum
// when it is met: the minimum only falls); tau = 2^-40 (|a| + max |b|)^2 bounds twice the difference between the bracket + |a|^2 and the
// reference sum ((a_0 - b_0)^2 + ...) + ... of 33 rounded terms (< 80 roundings of quantities <= (|a| + |b|)^2 on either side).  The kept
// targets -- one, unless descriptors are (nearly) equidistant -- are then evaluated in the reference form, in index order: same index, same
// d^2, ties to the lowest row, as feature_match_body.  A lane that met more than two candidates evaluates its whole share directly.
// Operand layout (mfma_ops_kernel): ops[tile][step 0..8][lane] with lane l <-> (row = 16 tile + (l & 15), k = 4 step + (l >> 4)), the layout
// both the A operand (rows = targets) and the B operand (columns = queries) of the instruction use: one coalesced 512-byte read per step.
typedef double fm_v4 __attribute__((ext_vector_type(4)));
constexpr int FM_NT = 4;             // query tiles of 16 per wave
constexpr double FM_TAU_REL = 9.094947017729282e-13;   // 2^-40
// Identical descriptors are common -- the points of a scan whose neighbourhoods hold a single other point all get the same one: groups of
// 50 - 70 rows in a 1 000-row scan -- and a query that is one of them ties with every target that is: dozens of exact evaluations behind the
// sweep.  A row that repeats an EARLIER row of its scan can never be the answer (same distance, higher index): it is taken out of the
// sweep's targets (its operand row becomes a padding row).  One block per scan: a hash table in LDS keeps the lowest row of every hash
// tag; a row whose tag's lowest row is an earlier one compares itself with that row bit by bit.
__global__ void __launch_bounds__(1024) dup_rows_kernel(const double* __restrict__ fpfh /* (ng,33) */, const unsigned int* __restrict__ scan_first,
                                                        unsigned char* __restrict__ dup /* (ng): 1 = repeats an earlier row of its scan */) {
    // open-addressing table in LDS: hash tag (high 32 bits) << 32 | lowest row seen with that tag; all ones = free
    constexpr unsigned int SLOTS = 2 * HYBRID_BRUTE_MAX;
    static_assert(SLOTS * 8 <= 65536 && (SLOTS & (SLOTS - 1)) == 0, "the table fits the block's LDS");
    __shared__ unsigned long long tab[SLOTS];
    const unsigned int base = scan_first[blockIdx.x], n = scan_first[blockIdx.x + 1] - base;   // (n <= HYBRID_BRUTE_MAX: checked by the caller)
    for (unsigned int i = threadIdx.x; i < SLOTS; i += 1024) tab[i] = ~0ull;
    __syncthreads();
    auto row_hash = [&](unsigned int j) {
        const unsigned long long* x = reinterpret_cast<const unsigned long long*>(fpfh + 33 * (size_t)(base + j));
        unsigned long long h = 0x9E3779B97F4A7C15ull;
        for (int k = 0; k < 33; ++k) { h ^= x[k]; h *= 0xD1B54A32D192ED03ull; h ^= h >> 29; }
        return h;
    };
    for (unsigned int j = threadIdx.x; j < n; j += 1024) {
        const unsigned long long h = row_hash(j), mine = (h & 0xffffffff00000000ull) | j;
        for (unsigned int slot = (unsigned int)h & (SLOTS - 1);; slot = (slot + 1) & (SLOTS - 1)) {
            const unsigned long long cur = tab[slot];
            if (cur == ~0ull) {
                if (atomicCAS(&tab[slot], ~0ull, mine) == ~0ull) break;
                --slot;   // somebody took it first: look at it again
                continue;
            }
            if ((cur >> 32) == (h >> 32)) { atomicMin(&tab[slot], mine); break; }   // same tag: the lowest row stays
        }
    }
    __syncthreads();
    for (unsigned int j = threadIdx.x; j < n; j += 1024) {
        const unsigned long long h = row_hash(j);
        unsigned int rep = j;
        for (unsigned int slot = (unsigned int)h & (SLOTS - 1);; slot = (slot + 1) & (SLOTS - 1)) {
            const unsigned long long cur = tab[slot];
            if (cur == ~0ull) break;
            if ((cur >> 32) == (h >> 32)) { rep = (unsigned int)cur; break; }
        }
        unsigned char d = 0;
        if (rep < j) {   // the same tag: the rows themselves decide (a colliding tag leaves the row a target: harmless)
            const unsigned long long* xi = reinterpret_cast<const unsigned long long*>(fpfh + 33 * (size_t)(base + rep));
            const unsigned long long* xj = reinterpret_cast<const unsigned long long*>(fpfh + 33 * (size_t)(base + j));
            bool same = true;
            for (int k = 0; k < 33; ++k) same = same && xi[k] == xj[k];
            d = same ? 1 : 0;
        }
        dup[base + j] = d;
    }
}

__global__ void __launch_bounds__(64) mfma_ops_kernel(const double* __restrict__ fpfh /* (ng,33) */, const unsigned int* __restrict__ scan_first, int n_scans,
                                                      const unsigned int* __restrict__ tile_first /* [n_scans + 1] */, const unsigned char* __restrict__ dup,
                                                      double* __restrict__ op_t, double* __restrict__ op_q,
                                                      double* __restrict__ norm2 /* (ng) */, unsigned long long* __restrict__ max_norm2 /* [n_scans], bits of a double */) {
    const unsigned int tile = blockIdx.x;
    const int lane = threadIdx.x;
    int lo = 0, hi = n_scans - 1;   // the scan that owns this tile
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tile_first[mid] <= tile) lo = mid;
        else hi = mid - 1;
    }
    const unsigned int base = scan_first[lo], n = scan_first[lo + 1] - base, lt = tile - tile_first[lo];
    const unsigned int row = 16u * lt + (unsigned int)(lane & 15);
    const bool live = row < n;
    const double* x = fpfh + 33 * (size_t)(base + row);
    double nn = 0.0;
    if (live)
        for (int k = 0; k < 33; ++k) nn += x[k] * x[k];
    if (live && lane < 16) {
        norm2[base + row] = nn;
        atomicMax(max_norm2 + lo, (unsigned long long)__double_as_longlong(nn));   // (non-negative doubles order like their bit patterns)
    }
#pragma unroll
    for (int st = 0; st < FM_STEPS; ++st) {
        const int k = 4 * st + (lane >> 4);
        double vt, vq;
        if (live) { vt = k < 33 ? -2.0 * x[k] : (k == 33 ? nn : 0.0); vq = k < 33 ? x[k] : (k == 33 ? 1.0 : 0.0); }
        else { vt = k == 33 ? 1e300 : 0.0; vq = 0.0; }   // a padding row never wins as a target, and is nobody's query
        if (live && dup[base + row]) vt = k == 33 ? 1e300 : 0.0;   // a repeated row: still a query, never a target
        op_t[((size_t)tile * FM_STEPS + st) * 64 + lane] = vt;
        op_q[((size_t)tile * FM_STEPS + st) * 64 + lane] = vq;
    }
}

// per scan: the row with the smallest squared norm, lowest row on ties (one block per scan)
__global__ void __launch_bounds__(256) min_norm_row_kernel(const double* __restrict__ norm2, const unsigned int* __restrict__ scan_first, unsigned int* __restrict__ min_row) {
    __shared__ double s_v[256];
    __shared__ unsigned int s_r[256];
    const unsigned int base = scan_first[blockIdx.x], n = scan_first[blockIdx.x + 1] - base;
    double v = DBL_MAX;
    unsigned int r = 0xffffffffu;
    for (unsigned int i = threadIdx.x; i < n; i += 256) {
        const double x = norm2[base + i];
        if (x < v) { v = x; r = i; }   // (ascending rows per thread: the first one met stays on ties)
    }
    s_v[threadIdx.x] = v; s_r[threadIdx.x] = r;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            const double ov = s_v[threadIdx.x + off];
            const unsigned int orow = s_r[threadIdx.x + off];
            if (ov < s_v[threadIdx.x] || (ov == s_v[threadIdx.x] && orow < s_r[threadIdx.x])) { s_v[threadIdx.x] = ov; s_r[threadIdx.x] = orow; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) min_row[blockIdx.x] = s_r[0];
}

__device__ static inline double fm_exact(const double* __restrict__ a, const double* __restrict__ b) {   // feature_match_body's sum, term by term
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 33; ++k) { const double d = a[k] - b[k]; s += d * d; }
    return s;
}

__global__ void __launch_bounds__(256) feature_match_mfma_jobs_kernel(const init_job* __restrict__ jobs, int mutual, int splits /* target splits = gridDim.y */) {
    const init_job J = jobs[blockIdx.z >> 1];
    const bool back = (blockIdx.z & 1) != 0;
    if (back && !mutual) return;
    const int na = back ? J.nb : J.na, nb = back ? J.na : J.nb;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int qt0 = ((int)blockIdx.x * 4 + wave) * FM_NT;   // this wave's first query tile
    if (qt0 * 16 >= na) return;
    const double* const A = back ? J.fb : J.fa;     // queries, reference layout
    const double* const B = back ? J.fa : J.fb;     // targets
    const double* const opq = back ? J.qb : J.qa;
    const double* const opt = back ? J.ta : J.tb;
    const double* const n2q = back ? J.n2b : J.n2a;
    const double* const n2t = back ? J.n2a : J.n2b;
    const unsigned int* const mrt = back ? J.mra : J.mrb;
    const double bmax = sqrt(*(back ? J.mxa : J.mxb));
    int* const idx_out = back ? J.ci_ba : J.ci_ab;
    double* const d2_out = back ? J.cd_ba : J.cd_ab;
    const int q_tiles = (na + 15) >> 4;
    double bq[FM_NT][FM_STEPS];
    double tau[FM_NT], m[FM_NT], hi[FM_NT];   // hi = m + tau, refreshed when m moves
    int c0[FM_NT], c1[FM_NT], cnt[FM_NT];
    bool zq[FM_NT];   // an all-zero query (the descriptor of an isolated point): its distance to target j is |b_j|^2 -- term for term the sum
                      // mfma_ops_kernel stored -- and it ties with every all-zero target: answered from min_norm_row_kernel's table
#pragma unroll
    for (int tt = 0; tt < FM_NT; ++tt) {
        const bool tile_ok = qt0 + tt < q_tiles;
#pragma unroll
        for (int st = 0; st < FM_STEPS; ++st) bq[tt][st] = tile_ok ? opq[((size_t)(qt0 + tt) * FM_STEPS + st) * 64 + lane] : 0.0;
        const int qi = (qt0 + tt) * 16 + (lane & 15);
        const double qn = qi < na ? sqrt(n2q[qi]) : 0.0;
        zq[tt] = splits == 1 && qi < na && qn == 0.0;
        tau[tt] = FM_TAU_REL * (qn + bmax) * (qn + bmax);
        m[tt] = DBL_MAX; hi[tt] = DBL_MAX; c0[tt] = c1[tt] = -1; cnt[tt] = 0;
    }
    // (one wave sweeps a whole split of the targets -- all of them by default: the exact evaluation behind the sweep is per (query, split))
    const long long per = ((nb + splits - 1) / splits + 15) / 16 * 16;
    const int tb = (int)((long long)blockIdx.y * per), te = (int)(tb + per < nb ? tb + per : nb);
    const int t_end = (te + 15) >> 4;
    double a_next[FM_STEPS];
#pragma unroll
    for (int st = 0; st < FM_STEPS; ++st) a_next[st] = (tb >> 4) < t_end ? opt[((size_t)(tb >> 4) * FM_STEPS + st) * 64 + lane] : 0.0;
    for (int t = tb >> 4; t < t_end; ++t) {
        double a[FM_STEPS];
#pragma unroll
        for (int st = 0; st < FM_STEPS; ++st) a[st] = a_next[st];
        if (t + 1 < t_end) {   // the next tile's operands are on their way while this one is multiplied
#pragma unroll
            for (int st = 0; st < FM_STEPS; ++st) a_next[st] = opt[((size_t)(t + 1) * FM_STEPS + st) * 64 + lane];
        }
        fm_v4 acc[FM_NT];
#pragma unroll
        for (int tt = 0; tt < FM_NT; ++tt) acc[tt] = fm_v4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int st = 0; st < FM_STEPS; ++st)
#pragma unroll
            for (int tt = 0; tt < FM_NT; ++tt) acc[tt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[st], bq[tt][st], acc[tt], 0, 0, 0);
        const int j0 = t * 16 + (lane >> 4);   // this lane's four target rows of the tile: j0, j0 + 4, j0 + 8, j0 + 12 (the D layout of the instruction)
        // (almost every tile holds nothing near a lane's running minimum: one comparison of the four values' minimum against m + tau decides)
#pragma unroll
        for (int tt = 0; tt < FM_NT; ++tt) {
            const double vm = vmin(vmin(acc[tt][0], acc[tt][1]), vmin(acc[tt][2], acc[tt][3]));
            if (vm <= hi[tt]) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double v = acc[tt][r];
                    const int j = j0 + 4 * r;
                    if (v < m[tt] - tau[tt]) { m[tt] = v; c0[tt] = j; cnt[tt] = 1; }
                    else if (v <= m[tt] + tau[tt]) {
                        if (cnt[tt] == 1) c1[tt] = j;
                        cnt[tt] = cnt[tt] < 3 ? cnt[tt] + 1 : 3;
                        m[tt] = v < m[tt] ? v : m[tt];
                    }
                }
                hi[tt] = m[tt] + tau[tt];
            }
        }
    }
    // ---- the candidates in the reference form; the four lanes of a query meet
#pragma unroll
    for (int tt = 0; tt < FM_NT; ++tt) {
        const int qi = (qt0 + tt) * 16 + (lane & 15);
        double best = DBL_MAX;
        int bj = -1;
        // only a lane whose share's minimum is within tau of the query's minimum over all four shares can hold the winner (usually one of four)
        double gm = m[tt];
        gm = vmin(gm, __shfl_xor(gm, 16, 64));
        gm = vmin(gm, __shfl_xor(gm, 32, 64));
        const bool need = qi < na && !zq[tt] && cnt[tt] >= 1 && m[tt] <= gm + tau[tt];
        if (!need) cnt[tt] = 0;
        if (zq[tt] && (lane >> 4) == 0) { bj = (int)*mrt; best = n2t[bj]; }
        if (need) {
            const double* const aq = A + 33 * (size_t)qi;
            if (cnt[tt] <= 2) {
                if (cnt[tt] >= 1 && c0[tt] < te) { best = fm_exact(aq, B + 33 * (size_t)c0[tt]); bj = c0[tt]; }
                if (cnt[tt] == 2 && c1[tt] < te) {
                    const double d = fm_exact(aq, B + 33 * (size_t)c1[tt]);
                    if (d < best) { best = d; bj = c1[tt]; }
                }
            }   // (cnt = 3: more than two candidates -- the second sweep below)
        }
        // (Nearly) equidistant descriptors are not rare: an isolated point has an all-zero descriptor, and every scan has a few -- a query
        // that is one ties with all of the target's.  Such a lane knows its share's final minimum now: the wave multiplies once more and the
        // lane evaluates, in index order, exactly the rows within tau of it (its whole share directly was 132 evaluations of 66 loads).
        if (__any(qi < na && cnt[tt] == 3)) {
            const bool mine = qi < na && cnt[tt] == 3;
            const double* const aq = A + 33 * (size_t)(qi < na ? qi : 0);
            double a2n[FM_STEPS];   // (operands one tile ahead, as in the first sweep: nine dependent reads per tile were 0.7 ms for ONE such wave)
#pragma unroll
            for (int st = 0; st < FM_STEPS; ++st) a2n[st] = (tb >> 4) < t_end ? opt[((size_t)(tb >> 4) * FM_STEPS + st) * 64 + lane] : 0.0;
            for (int t = tb >> 4; t < t_end; ++t) {
                double a2[FM_STEPS];
#pragma unroll
                for (int st = 0; st < FM_STEPS; ++st) a2[st] = a2n[st];
                if (t + 1 < t_end) {
#pragma unroll
                    for (int st = 0; st < FM_STEPS; ++st) a2n[st] = opt[((size_t)(t + 1) * FM_STEPS + st) * 64 + lane];
                }
                fm_v4 acc2 = fm_v4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int st = 0; st < FM_STEPS; ++st) acc2 = __builtin_amdgcn_mfma_f64_16x16x4f64(a2[st], bq[tt][st], acc2, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int j = t * 16 + (lane >> 4) + 4 * r;
                    if (mine && j < te && acc2[r] <= m[tt] + tau[tt]) {
                        const double d = fm_exact(aq, B + 33 * (size_t)j);
                        if (d < best) { best = d; bj = j; }
                    }
                }
            }
        }
#pragma unroll
        for (int off = 16; off < 64; off <<= 1) {
            const double od = __shfl_xor(best, off, 64);
            const int oj = __shfl_xor(bj, off, 64);
            if (oj >= 0 && (bj < 0 || od < best || (od == best && oj < bj))) { best = od; bj = oj; }
        }
        if (qi < na && (lane >> 4) == 0) { idx_out[(long long)blockIdx.y * na + qi] = bj; d2_out[(long long)blockIdx.y * na + qi] = best; }
    }
}

__global__ void __launch_bounds__(256) feature_match_merge_jobs_kernel(const init_job* __restrict__ jobs, int mutual, int splits) {
    const init_job J = jobs[blockIdx.y >> 1];
    const bool back = (blockIdx.y & 1) != 0;
    if (back && !mutual) return;
    const long long na = back ? J.nb : J.na;
    feature_match_merge_body(back ? J.ci_ba : J.ci_ab, back ? J.cd_ba : J.cd_ab, na, splits, back ? J.ji : J.ij, back ? J.dba : J.dab, blockIdx.x);
}
__global__ void __launch_bounds__(256) corr_build_jobs_kernel(const init_job* __restrict__ jobs, int mutual, int min_mutual, int max_iteration) {
    __shared__ corr_lds s_L;
    const init_job J = jobs[blockIdx.x];
    corr_build_body(J.ij, J.ji, J.na, mutual, min_mutual, J.corr, J.m, &s_L);
    __syncthreads();   // (the count is written by thread 0, which also initialises the loop state)
    ransac_init(J.st, J.m, max_iteration);
}

// ------------------------------------------------------------------ host side
constexpr int MIN_MUTUAL = 9;   // fewer mutual correspondences than this: the one-way set (see corr_build_body)

int pcr_feature_match_device(pcr_ctx* ctx, const double* dA, long long na, const double* dB, long long nb, int dim, int* d_idx, double* d_d2) {
    const unsigned grid = (unsigned)((na + 255) / 256);
    const size_t lds = sizeof(double) * FM_TILE * dim;
    // enough blocks to fill the chip: split the targets when there are few query blocks
    int splits = (int)((4ll * ctx->cu_count + grid - 1) / grid);
    const long long max_splits = (nb + FM_TILE - 1) / FM_TILE;
    if (splits > max_splits) splits = (int)max_splits;
    if (splits < 1) splits = 1;
    if (splits > 256) splits = 256;
    const long long per = ((nb + splits - 1) / splits + FM_TILE - 1) / FM_TILE * FM_TILE;
    splits = (int)((nb + per - 1) / per);
    pcr_dev_block ci(ctx), cd(ctx);
    int rc;
    if ((rc = ci.alloc(sizeof(int) * na * splits)) || (rc = cd.alloc(sizeof(double) * na * splits))) return rc;
    const auto match_k = dim == 33 ? feature_match_kernel<33> : feature_match_kernel<0>;
    hipLaunchKernelGGL(match_k, dim3(grid, splits), dim3(256), lds, ctx->stream, dA, na, dB, nb, dim, per, ci.as<int>(), cd.as<double>());
    hipLaunchKernelGGL(feature_match_merge_kernel, dim3(grid), dim3(256), 0, ctx->stream, (const int*)ci.as<int>(), (const double*)cd.as<double>(), na, splits, d_idx, d_d2);
    PCR_HIP(ctx, hipGetLastError());
    return PCR_OK;
}

void pcr_corr_build(pcr_ctx* ctx, const int* ij, const int* ji, int na, int mutual, int* corr, int* d_m) {
    hipLaunchKernelGGL(corr_build_kernel, dim3(1), dim3(256), 0, ctx->stream, ij, ji, na, mutual, MIN_MUTUAL, corr, d_m);
}

void pcr_match_operands(pcr_ctx* ctx, const double* fpfh, const unsigned int* scan_first, int n_scans, size_t tiles, const unsigned int* tile_first,
                        unsigned char* dup, double* op_t, double* op_q, double* norm2, unsigned long long* max_norm2, unsigned int* min_row) {
    hipLaunchKernelGGL(dup_rows_kernel, dim3((unsigned)n_scans), dim3(1024), 0, ctx->stream, fpfh, scan_first, dup);
    if (tiles)
        hipLaunchKernelGGL(mfma_ops_kernel, dim3((unsigned)tiles), dim3(64), 0, ctx->stream, fpfh, scan_first, n_scans, tile_first, (const unsigned char*)dup, op_t, op_q,
                           norm2, max_norm2);
    hipLaunchKernelGGL(min_norm_row_kernel, dim3((unsigned)n_scans), dim3(256), 0, ctx->stream, (const double*)norm2, scan_first, min_row);
}

void pcr_match_jobs(pcr_ctx* ctx, const init_job* d_jobs, int nj, int max_n, int mutual, int max_iteration) {
    const unsigned qb = (unsigned)((max_n + 255) / 256);
    // (matrix-core sweep: one split -- 4 waves per 256 queries and direction -- unless a pair or two are all there is)
    const int mfma_splits = (long long)nj * 2 * qb * 4 >= (long long)ctx->cu_count ? 1 : (JOB_SPLITS < 4 ? JOB_SPLITS : 4);
    hipLaunchKernelGGL(feature_match_mfma_jobs_kernel, dim3(qb, mfma_splits, 2 * nj), dim3(256), 0, ctx->stream, d_jobs, mutual, mfma_splits);
    hipLaunchKernelGGL(feature_match_merge_jobs_kernel, dim3(qb, 2 * nj), dim3(256), 0, ctx->stream, d_jobs, mutual, mfma_splits);
    hipLaunchKernelGGL(corr_build_jobs_kernel, dim3(nj), dim3(256), 0, ctx->stream, d_jobs, mutual, MIN_MUTUAL, max_iteration);
}

extern "C" int pcr_feature_match(pcr_ctx* ctx, const double* queries, int64_t nq, const double* targets, int64_t nt, int dim, int32_t* idx_out, double* d2_out) {
    if (!ctx || !queries || !targets || !idx_out || dim < 1 || dim > 512) return PCR_E_INVALID;
    if (nq <= 0 || nt <= 0) return PCR_E_EMPTY;
    hipSetDevice(ctx->device);
    pcr_dev_block a(ctx), b(ctx), di(ctx), dd(ctx);
    int rc;
    if ((rc = a.alloc(sizeof(double) * dim * nq)) || (rc = b.alloc(sizeof(double) * dim * nt)) || (rc = di.alloc(sizeof(int) * nq)) || (rc = dd.alloc(sizeof(double) * nq))) return rc;
    PCR_HIP(ctx, hipMemcpyAsync(a.p, queries, sizeof(double) * dim * nq, hipMemcpyHostToDevice, ctx->stream));
    PCR_HIP(ctx, hipMemcpyAsync(b.p, targets, sizeof(double) * dim * nt, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = pcr_feature_match_device(ctx, a.as<double>(), nq, b.as<double>(), nt, dim, di.as<int>(), dd.as<double>()))) return rc;
    PCR_HIP(ctx, hipMemcpyAsync(idx_out, di.p, sizeof(int) * nq, hipMemcpyDeviceToHost, ctx->stream));
    if (d2_out) PCR_HIP(ctx, hipMemcpyAsync(d2_out, dd.p, sizeof(double) * nq, hipMemcpyDeviceToHost, ctx->stream));
    PCR_HIP(ctx, pcr_sync(ctx->stream));
    return PCR_OK;
}
