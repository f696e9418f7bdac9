// Descriptors of the global initialisation in front of ICP -- the Open3D calls of Registration/main.py:33-47:
//   pcr_normals_hybrid   estimate_normals(KDTreeSearchParamHybrid(radius, max_nn))      main.py:39-40
//   pcr_fpfh             compute_fpfh_feature(pcd, KDTreeSearchParamHybrid(radius, max_nn)) main.py:44-46
//   pcr_fpfh_rows        the same descriptors at chosen rows only (keypoints over the cloud as search surface), bit for bit
// Open3D is a third-party dependency that is absent here and unpinned in the reference: the algorithms below
// follow its published behaviour (FPFH of Rusu et al. 2009 as implemented by Open3D >= 0.12: 3 x 11 bins,
// increments 100/(k-1), neighbour SPFH weighted by 1/d^2 and renormalised to 100 per sub-histogram).
// "Parity unpinned": no output of the reference exists for this stage (its RANSAC is randomised).
//
// Hybrid neighbourhood = the up-to-max_nn nearest points with d^2 < radius^2, ordered by (d^2, row).  One
// 64-lane wave per point: the 3x3x3 block of a grid with cell = radius is scanned, candidates inside the
// sphere are compacted into LDS (ballot + prefix), bitonic-sorted, truncated.  More than NB_CAP candidates
// inside the sphere: the radius is first bisected down to a value that keeps between max_nn and NB_CAP.
#include <cfloat>
#include <cmath>
#include <cstring>
#include "pcr_grid_dev.h"
#include "pcr_linalg.h"
#include "pcr_global_dev.h"
#include "pcr_sort.h"
#include "pcr_pair_features.h"

struct __attribute__((aligned(16))) nb_entry {
    double d2;
    unsigned int pos;  // position in the index's sorted order
    unsigned int id;   // caller row
};

__device__ static inline bool nb_less(const nb_entry& a, const nb_entry& b) { return a.d2 < b.d2 || (a.d2 == b.d2 && a.id < b.id); }

// blockDim.x == 64.  Returns the neighbour count (<= max_nn), entries sorted in nb[0..count); -1 = cannot bound the set.
// The 27 cells are looked up by 27 lanes AT ONCE (one lane walking them one after the other paid 27 dependent round trips per
// point), the non-empty ones become a flat list of ranges (cell_s / cell_o: start and exclusive point offset) and the 64 lanes
// stride over the concatenation, so a scan is ceil(points / 64) round trips whatever the cells' sizes.
// CAP < NB_CAP: a block with a small candidate array (more blocks per CU); a sphere that holds more returns -2 and the point is done
// again by the block with the full array.
// (The cell lookup and the ballot compaction below are this function's own copies of ball_cell_run / wave_compact_slot of
// pcr_ball_visit.h: with either of them called from here the same registers are allocated differently and hybrid_normals_kernel
// measured 1.6 % slower on the 120 000-point scan (8.57 against 8.43 ms, medians of five alternating processes) -- profiles/ball_walk_resources.md.)
template <int CAP>
struct hybrid_lds_t {
    nb_entry nb[CAP];
    unsigned int cell_s[28], cell_o[28];
};
typedef hybrid_lds_t<NB_CAP> hybrid_lds;
template <int CAP>
__device__ static int gather_hybrid(const pcr_grid_view& gv, double qx, double qy, double qz, double r2, int max_nn, hybrid_lds_t<CAP>* L) {
    nb_entry* const nb = L->nb;
    const int lane = threadIdx.x;
    bool clamped = false;
    const int cx = cell_coord(qx, gv.lo[0], gv.inv_cell0, &clamped);
    const int cy = cell_coord(qy, gv.lo[1], gv.inv_cell0, &clamped);
    const int cz = cell_coord(qz, gv.lo[2], gv.inv_cell0, &clamped);
    unsigned int s = 0, e = 0;
    bool has = false;
    if (gv.levels == 0) {
        // no grid (a cloud of a few thousand points, see brute_view): the whole cloud is the one "cell".  The sphere test, the order
        // (d^2, row) and the cut at max_nn make the list -- the same list whatever superset of the sphere was scanned.
        has = lane == 0;
        e = (unsigned int)gv.n;
    } else if (lane < 27) {
        const unsigned int nx = (unsigned int)(cx + lane % 3 - 1), ny = (unsigned int)(cy + (lane / 3) % 3 - 1), nz = (unsigned int)(cz + lane / 9 - 1);
        if (nx <= (unsigned int)PCR_COORD_MAX && ny <= (unsigned int)PCR_COORD_MAX && nz <= (unsigned int)PCR_COORD_MAX)
            has = lookup_cell(gv.table[0], gv.mask[0], nx, ny, nz, &s, &e);
    }
    const unsigned long long m_has = __ballot(has);
    const int n_cells = __popcll(m_has);
    unsigned int inc = has ? e - s : 0u;
#pragma unroll
    for (int off = 1; off < 32; off <<= 1) {   // lanes 0..26 hold the counts
        const unsigned int o = __shfl_up(inc, off, 64);
        if (lane >= off) inc += o;
    }
    const unsigned int total = __shfl(inc, 31, 64);
    if (has) {
        const int r = __popcll(m_has & ((1ull << lane) - 1ull));
        L->cell_s[r] = s;
        L->cell_o[r] = inc - (e - s);
    }
    __syncthreads();
    auto scan = [&](double T, bool store) -> int {
        int found = 0;
        for (unsigned int t0 = 0; t0 < total; t0 += 64) {
            const unsigned int t = t0 + lane;
            bool keep = false;
            nb_entry en;
            en.d2 = 0.0; en.pos = 0; en.id = 0;
            if (t < total) {
                int lo = 0, hi = n_cells - 1;
                while (lo < hi) {
                    const int mid = (lo + hi + 1) >> 1;
                    if (L->cell_o[mid] <= t) lo = mid;
                    else hi = mid - 1;
                }
                const unsigned int j = L->cell_s[lo] + (t - L->cell_o[lo]);
                const pcr_pt b = gv.pts[j];
                en.d2 = dist2(qx, qy, qz, b);
                en.pos = j;
                en.id = (unsigned int)b.id;
                keep = en.d2 < T;
            }
            const unsigned long long m = __ballot(keep);
            const int rank = __popcll(m & ((1ull << lane) - 1ull));
            if (store && keep && found + rank < CAP) nb[found + rank] = en;
            found += __popcll(m);
        }
        return found;
    };
    int cnt = scan(r2, true);
    if (CAP < NB_CAP && cnt > CAP) return -2;
    if (cnt > NB_CAP) {
        unsigned long long lo = 0, hi = (unsigned long long)__double_as_longlong(r2);
        bool found = false;
        double T = r2;
        for (int it = 0; it < 70 && hi - lo > 1; ++it) {
            const unsigned long long mid = lo + (hi - lo) / 2;
            T = __longlong_as_double((long long)mid);
            const int c = scan(T, false);
            if (c > NB_CAP) hi = mid;
            else if (c < max_nn) lo = mid;
            else { found = true; break; }
        }
        if (!found) return -1;
        __syncthreads();
        cnt = scan(T, true);
    }
    int P = 64;
    while (P < cnt) P <<= 1;
    for (int i = cnt + lane; i < P; i += 64) { nb[i].d2 = DBL_MAX; nb[i].pos = POS_NONE; nb[i].id = 0xffffffffu; }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = lane; i < P; i += 64) {
                const int l = i ^ j;
                if (l > i) {
                    const nb_entry a = nb[i], b = nb[l];
                    const bool up = (i & k) == 0;
                    if (up ? nb_less(b, a) : nb_less(a, b)) { nb[i] = b; nb[l] = a; }
                }
            }
            __syncthreads();
        }
    return cnt < max_nn ? cnt : max_nn;
}

// symmetric 3x3 Jacobi: eigenvector of the smallest eigenvalue
__device__ static void smallest_eigvec(const double S[6], double n[3]) {
    double A[3][3] = {{S[0], S[1], S[2]}, {S[1], S[3], S[4]}, {S[2], S[4], S[5]}};
    double Q[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    pcr::sym3_jacobi(A, Q);
    // (selects on values read into scalars first, not Q[i][m] with a run-time m: a dynamically indexed local array lives in scratch
    // memory -- 112 bytes per lane for this kernel)
    const double a0 = A[0][0], a1 = A[1][1], a2 = A[2][2];
    const bool m1 = a1 < a0;
    const double am = m1 ? a1 : a0;
    const bool m2 = a2 < am;
    const double q00 = Q[0][0], q01 = Q[0][1], q02 = Q[0][2], q10 = Q[1][0], q11 = Q[1][1], q12 = Q[1][2], q20 = Q[2][0], q21 = Q[2][1], q22 = Q[2][2];
    n[0] = m2 ? q02 : (m1 ? q01 : q00);
    n[1] = m2 ? q12 : (m1 ? q11 : q10);
    n[2] = m2 ? q22 : (m1 ? q21 : q20);
}

// ------------------------------------------------------------ hybrid normals
// returns false when the point has to be done again with the full candidate array
// the normal of a point from the covariance S of its neighbourhood (cnt < 3: Open3D's (0, 0, 1)); the same arithmetic whoever runs it
__device__ static inline void normal_from_cov(const double S[6], int cnt, const pcr_pt& p, int orient, double vx, double vy, double vz, double nrm[3]) {
    nrm[0] = 0.0; nrm[1] = 0.0; nrm[2] = 1.0;
    if (cnt < 3) return;
    smallest_eigvec(S, nrm);
    const double len = sqrt(nrm[0] * nrm[0] + nrm[1] * nrm[1] + nrm[2] * nrm[2]);
    if (len == 0.0 || !(len == len)) { nrm[0] = 0; nrm[1] = 0; nrm[2] = 1; }
    else if (orient) {
        const double d = nrm[0] * (vx - p.x) + nrm[1] * (vy - p.y) + nrm[2] * (vz - p.z);
        if (d < 0) { nrm[0] = -nrm[0]; nrm[1] = -nrm[1]; nrm[2] = -nrm[2]; }
    }
}
// `cov` (or null): the covariance and the count go to cov[7 * row .. + 7) and the normal is left to normals_finish_kernel -- one THREAD
// per point there: the Jacobi sweeps are ~1 000 dependent instructions, 40 % of this kernel's when a whole wave runs them for one point
template <int CAP>
__device__ static bool normals_body(const pcr_grid_view& gv, const pcr_pt& p, double r2, int max_nn, int orient, double vx, double vy, double vz,
                                    double* __restrict__ normals /* (n,3) by row */, int* __restrict__ fail, hybrid_lds_t<CAP>* L, double* __restrict__ cov = nullptr) {
    nb_entry* const nb = L->nb;
    const int cnt = gather_hybrid<CAP>(gv, p.x, p.y, p.z, r2, max_nn, L);
    if (cnt == -2) return false;
    if (cnt < 0) {
        if (threadIdx.x == 0) { atomicAdd(fail, 1); if (cov) cov[7 * p.id + 6] = 0.0; }
        return true;
    }
    double S[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (cnt >= 3) {
        // cumulants about the query point (Open3D accumulates raw coordinates; centring first is the same
        // covariance with less cancellation)
        double c[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int k = threadIdx.x; k < cnt; k += 64) {
            const pcr_pt b = gv.pts[nb[k].pos];
            const double x = b.x - p.x, y = b.y - p.y, z = b.z - p.z;
            c[0] += x; c[1] += y; c[2] += z;
            c[3] += x * x; c[4] += x * y; c[5] += x * z; c[6] += y * y; c[7] += y * z; c[8] += z * z;
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) c[k] = wave_sum_all(c[k]) / (double)cnt;
        S[0] = c[3] - c[0] * c[0]; S[1] = c[4] - c[0] * c[1]; S[2] = c[5] - c[0] * c[2];
        S[3] = c[6] - c[1] * c[1]; S[4] = c[7] - c[1] * c[2]; S[5] = c[8] - c[2] * c[2];
    }
    if (cov) {
        if (threadIdx.x < 7) {
            const double v = threadIdx.x == 0 ? S[0] : threadIdx.x == 1 ? S[1] : threadIdx.x == 2 ? S[2] : threadIdx.x == 3 ? S[3] : threadIdx.x == 4 ? S[4] : threadIdx.x == 5 ? S[5] : (double)cnt;
            cov[7 * p.id + threadIdx.x] = v;
        }
        return true;
    }
    double nrm[3];
    normal_from_cov(S, cnt, p, orient, vx, vy, vz, nrm);
    const double n0 = nrm[0], n1 = nrm[1], n2 = nrm[2];
    if (threadIdx.x < 3) normals[3 * p.id + threadIdx.x] = threadIdx.x == 0 ? n0 : (threadIdx.x == 1 ? n1 : n2);
    return true;
}

__global__ void __launch_bounds__(64) hybrid_normals_kernel(pcr_grid_view gv, long long n, double r2, int max_nn, int orient, double vx, double vy,
                                                            double vz, double* __restrict__ normals /* (n,3) by row */, int* __restrict__ fail) {
    __shared__ hybrid_lds s_L;
    const long long i = blockIdx.x;
    if (i >= n) return;
    const pcr_pt p = gv.pts[i];
    normals_body<NB_CAP>(gv, p, r2, max_nn, orient, vx, vy, vz, normals, fail, &s_L);
}

__device__ static inline unsigned int scans_block_view(const scans_view& V, long long i, pcr_grid_view* gv) {
    const unsigned int s = V.vsid[i], base = V.scan_first[s];
    gv->pts = V.down + base;
    gv->n = (long long)(V.scan_first[s + 1] - base);
    gv->levels = 0;
    gv->lo[0] = gv->lo[1] = gv->lo[2] = 0.0;
    gv->cell0 = 1.0; gv->inv_cell0 = 1.0;
    return base;
}
// Two launches per stage: every point with a SMALL candidate array (16 blocks and more per CU instead of 9: a block is a chain of round
// trips and LDS sorts, its throughput is how many run side by side), then the few whose sphere holds more, from the list the first left
// (`todo` / `todo_count`; a fixed grid strides over it -- its length is only known on the device).
template <int CAP>
__global__ void __launch_bounds__(64) normals_scans_kernel(scans_view V, long long ng, double r2, int max_nn, double* __restrict__ normals /* (ng,3) */, int* __restrict__ fail,
                                                           const unsigned int* __restrict__ todo, const unsigned int* __restrict__ todo_count, unsigned int* __restrict__ redo,
                                                           unsigned int* __restrict__ redo_count, double* __restrict__ cov /* (ng,7): covariance + count; the normals follow in normals_finish_kernel */) {
    __shared__ hybrid_lds_t<CAP> s_L;
    const long long n_do = todo ? (long long)*todo_count : ng;
    for (long long t = blockIdx.x; t < n_do; t += gridDim.x) {
        const long long i = todo ? (long long)todo[t] : t;
        pcr_grid_view gv;
        const unsigned int base = scans_block_view(V, i, &gv);
        const pcr_pt p = V.down[i];
        const bool done = normals_body<CAP>(gv, p, r2, max_nn, 1, 0.0, 0.0, 0.0, normals + 3 * (size_t)base, fail, &s_L, cov + 7 * (size_t)base);
        if (!done && threadIdx.x == 0) redo[atomicAdd(redo_count, 1u)] = (unsigned int)i;
        __syncthreads();   // (the candidate array is reused by the next point)
    }
}
// one thread per down-sampled point of the chunk: covariance -> normal (towards the origin, as pcr_preprocess asks)
__global__ void __launch_bounds__(256) normals_finish_kernel(scans_view V, long long ng, const double* __restrict__ cov, double* __restrict__ normals) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ng) return;
    const pcr_pt p = V.down[i];   // (record base + r is row r: cov and normals of point i sit at i)
    double S[6], nrm[3];
#pragma unroll
    for (int k = 0; k < 6; ++k) S[k] = cov[7 * i + k];
    normal_from_cov(S, (int)cov[7 * i + 6], p, 1, 0.0, 0.0, 0.0, nrm);
    normals[3 * i] = nrm[0]; normals[3 * i + 1] = nrm[1]; normals[3 * i + 2] = nrm[2];
}

// ---------------------------------------------------------------------- SPFH
// (the Darboux frame pair_features and the bin rule clamp_bin: pcr_pair_features.h, shared with the PCL-rule SPFH of pcr_fpfh_pcl.hip)

// Where ONE row's results go.  The full pass keeps every row's list for fpfh_kernel (LISTS); the rows pass (below) keeps only its
// SPFH, in a compact block.  The destination and the list store are the only differences: the pair loop, the binning, the skip of
// list entry 0 and the repeated-addition scaling exist once.
struct spfh_dest {
    double* __restrict__ spfh;                                                               // 33
    unsigned int* __restrict__ nb_id; double* __restrict__ nb_d2; int* __restrict__ nb_cnt;    // (max_nn) twice, one count; unused without LISTS
};
__device__ static inline spfh_dest spfh_dest_by_row(long long row, int max_nn, double* spfh, unsigned int* nb_id, double* nb_d2, int* nb_cnt) {
    return spfh_dest{spfh + 33 * row, nb_id + row * max_nn, nb_d2 + row * max_nn, nb_cnt + row};
}
template <int CAP, bool LISTS>
__device__ static bool spfh_body(const pcr_grid_view& gv, const pcr_pt& p, double r2, int max_nn, const double* __restrict__ normals /* by row */, const spfh_dest& out,
                                 int* __restrict__ fail, hybrid_lds_t<CAP>* L, int* hist /* LDS, 33 */) {
    nb_entry* const nb = L->nb;
    if (threadIdx.x < 33) hist[threadIdx.x] = 0;
    const int cnt = gather_hybrid<CAP>(gv, p.x, p.y, p.z, r2, max_nn, L);  // ends with a barrier
    if (cnt == -2) return false;
    // (an empty list: the FPFH launch behind this one reads every point's count -- and walks that many entries -- before the host sees the fail word)
    if (cnt < 0) { if (threadIdx.x == 0) { atomicAdd(fail, 1); if (LISTS) *out.nb_cnt = 0; } return true; }
    const double p1[3] = {p.x, p.y, p.z};
    const double n1[3] = {normals[3 * p.id], normals[3 * p.id + 1], normals[3 * p.id + 2]};
    for (int k = threadIdx.x; k < cnt; k += 64) {
        const nb_entry en = nb[k];
        if (LISTS) { out.nb_id[k] = en.id; out.nb_d2[k] = en.d2; }
        if (k == 0) continue;  // the query point itself (or a duplicate of it)
        const pcr_pt b = gv.pts[en.pos];
        const double p2[3] = {b.x, b.y, b.z};
        const double n2[3] = {normals[3 * (long long)en.id], normals[3 * (long long)en.id + 1], normals[3 * (long long)en.id + 2]};
        double f[3];
        pair_features(p1, n1, p2, n2, f);
        int bins[3];
        pair_bins(f, bins);
        atomicAdd(&hist[bins[0]], 1);
        atomicAdd(&hist[bins[1]], 1);
        atomicAdd(&hist[bins[2]], 1);
    }
    __syncthreads();
    if (LISTS && threadIdx.x == 0) *out.nb_cnt = cnt;
    if (threadIdx.x < 33) {
        double v = 0.0;
        if (cnt > 1) {
            const double incr = 100.0 / (double)(cnt - 1);
            for (int c = 0; c < hist[threadIdx.x]; ++c) v += incr;  // repeated addition, like the reference library
        }
        out.spfh[threadIdx.x] = v;
    }
    return true;
}

__global__ void __launch_bounds__(64)
spfh_kernel(pcr_grid_view gv, long long n, double r2, int max_nn, const double* __restrict__ normals /* by row */, double* __restrict__ spfh /* (n,33) by row */,
            unsigned int* __restrict__ nb_id /* (n,max_nn) by row */, double* __restrict__ nb_d2, int* __restrict__ nb_cnt, int* __restrict__ fail) {
    __shared__ hybrid_lds s_L;
    __shared__ int hist[33];
    const long long i = blockIdx.x;
    if (i >= n) return;
    const pcr_pt p = gv.pts[i];
    spfh_body<NB_CAP, true>(gv, p, r2, max_nn, normals, spfh_dest_by_row(p.id, max_nn, spfh, nb_id, nb_d2, nb_cnt), fail, &s_L, hist);
}

template <int CAP>
__global__ void __launch_bounds__(64)
spfh_scans_kernel(scans_view V, long long ng, double r2, int max_nn, const double* __restrict__ normals, double* __restrict__ spfh, unsigned int* __restrict__ nb_id,
                  double* __restrict__ nb_d2, int* __restrict__ nb_cnt, int* __restrict__ fail, const unsigned int* __restrict__ todo,
                  const unsigned int* __restrict__ todo_count, unsigned int* __restrict__ redo, unsigned int* __restrict__ redo_count) {
    __shared__ hybrid_lds_t<CAP> s_L;
    __shared__ int hist[33];
    const long long n_do = todo ? (long long)*todo_count : ng;
    for (long long t = blockIdx.x; t < n_do; t += gridDim.x) {
        const long long i = todo ? (long long)todo[t] : t;
        pcr_grid_view gv;
        const size_t base = scans_block_view(V, i, &gv);
        const pcr_pt p = V.down[i];
        const bool done = spfh_body<CAP, true>(gv, p, r2, max_nn, normals + 3 * base,
                                               spfh_dest_by_row(p.id, max_nn, spfh + 33 * base, nb_id + base * (size_t)max_nn, nb_d2 + base * (size_t)max_nn, nb_cnt + base), fail, &s_L, hist);
        if (!done && threadIdx.x == 0) redo[atomicAdd(redo_count, 1u)] = (unsigned int)i;
        __syncthreads();
    }
}

// ---------------------------------------------------------------------- FPFH
// One wave per point, lane = histogram bin (33 of 64).  The neighbour list (row, d^2) goes through LDS first, so the SPFH rows
// of four neighbours are requested together instead of one dependent chain id -> row per neighbour; every term is spfh / d^2
// (a true division, as in Open3D); the three renormalising sums are taken over the lanes of each 11-bin block at the end.
// `i`: the list (and the count) to walk; `self`: the SPFH row of the point itself; `fpfh`: its 33 outputs.  SLOT: the SPFH block is
// compact and slot[row] says where a row's histogram sits (the rows pass below) -- the rows are translated on their way into LDS, the
// sums behind that are the same instructions in the same order.
template <bool SLOT>
__device__ static void fpfh_body(const long long i, const long long self, int max_nn, const double* __restrict__ spfh, const unsigned int* __restrict__ slot,
                                 const unsigned int* __restrict__ nb_id, const double* __restrict__ nb_d2, const int* __restrict__ nb_cnt, double* __restrict__ fpfh /* 33 */,
                                 unsigned int* s_id, double* s_d2, double* s_acc) {
    const int cnt = nb_cnt[i];
    const int lane = threadIdx.x;
    for (int k = lane; k < cnt; k += 64) {
        const unsigned int id = nb_id[i * max_nn + k];
        s_id[k] = SLOT ? slot[id] : id;
        s_d2[k] = nb_d2[i * max_nn + k];
    }
    __syncthreads();
    double acc = 0.0;
    if (cnt > 1 && lane < 33) {
        int k = 1;
        for (; k + 4 <= cnt; k += 4) {
            double v[4], d[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { d[u] = s_d2[k + u]; v[u] = spfh[33 * (long long)s_id[k + u] + lane]; }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (d[u] != 0.0) acc += v[u] / d[u];
        }
        for (; k < cnt; ++k) {
            const double d = s_d2[k];
            if (d != 0.0) acc += spfh[33 * (long long)s_id[k] + lane] / d;
        }
        s_acc[lane] = acc;
    }
    __syncthreads();
    if (lane < 33) {
        double v = 0.0;
        if (cnt > 1) {
            const int g = lane / 11;
            double sum = 0.0;
#pragma unroll
            for (int j = 0; j < 11; ++j) sum += s_acc[11 * g + j];
            v = acc * (sum != 0.0 ? 100.0 / sum : 0.0) + spfh[33 * self + lane];
        }
        fpfh[lane] = v;
    }
}

__global__ void __launch_bounds__(64)
fpfh_kernel(long long n, int max_nn, const double* __restrict__ spfh, const unsigned int* __restrict__ nb_id, const double* __restrict__ nb_d2,
            const int* __restrict__ nb_cnt, double* __restrict__ fpfh /* (n,33) by row */) {
    __shared__ unsigned int s_id[NB_CAP];
    __shared__ double s_d2[NB_CAP];
    __shared__ double s_acc[33];
    const long long i = blockIdx.x;
    if (i >= n) return;
    fpfh_body<false>(i, i, max_nn, spfh, nullptr, nb_id, nb_d2, nb_cnt, fpfh + 33 * i, s_id, s_d2, s_acc);
}

// (the records of a scan sit in row order: record base + r is row r)
template <int CAP>   // >= max_nn (a list never holds more)
__global__ void __launch_bounds__(64)
fpfh_scans_kernel(scans_view V, long long ng, int max_nn, const double* __restrict__ spfh, const unsigned int* __restrict__ nb_id, const double* __restrict__ nb_d2,
                  const int* __restrict__ nb_cnt, double* __restrict__ fpfh) {
    __shared__ unsigned int s_id[CAP];
    __shared__ double s_d2[CAP];
    __shared__ double s_acc[33];
    const long long i = blockIdx.x;
    if (i >= ng) return;
    const size_t base = V.scan_first[V.vsid[i]];
    const long long r = i - (long long)base;
    fpfh_body<false>(r, r, max_nn, spfh + 33 * base, nullptr, nb_id + base * (size_t)max_nn, nb_d2 + base * (size_t)max_nn, nb_cnt + base, fpfh + 33 * (size_t)i, s_id, s_d2, s_acc);
}

// -------------------------------------------------------------- FPFH at chosen rows
// The descriptor of a row needs its own list and SPFH and the SPFH of the rows in that list -- at most max_nn + 1 rows -- so m chosen
// rows need at most m (max_nn + 1) histograms, not n.  Four launches and a compaction on the stream:
//   fpfh_rows_lists_kernel   one wave per ENTRY of `rows` (any order, repeats allowed): its hybrid list -> an (m,max_nn) block, and the
//                            word need[row] = 1 for every row of the list and for the entry's own row (plain stores of the same
//                            constant: several waves may write one word, there is nothing to lose)
//   rocprim::select          the marked rows, ascending, and their number M (it stays on the device; the launches behind it are sized by
//                            the bound min(n, m (max_nn + 1)) that the host knows)
//   spfh_rows_kernel         wave k < M: list and histogram of marked row k by spfh_body -> spfh[k]; need[row] becomes slot[row] = k
//   fpfh_rows_kernel         fpfh_body over the m stored lists, SPFH rows found through slot[]
// The same bits as the rows of the full pass, because nothing a row's result is made of depends on which other rows are computed:
//   a list     is a function of the query's coordinates, the searched records, r^2, max_nn and the order (d^2, row) -- gather_hybrid
//              on the same view (hybrid_space::open) whichever kernel calls it;
//   an SPFH    is integer counts over that list, then count additions of one increment: spfh_body both times;
//   an FPFH    adds spfh / d^2 in list order: fpfh_body both times.
// The entry's own row is marked besides its list: with max_nn or more exact duplicates of lower row in front of it a row is not in its
// own list, and fpfh_body still adds the row's own SPFH.  Without such duplicates M is the size of the union of the lists.
// A record's position is not its row on a re-laid cloud or in a grid index's order: row_pos_kernel writes the table row -> position
// for those (4 n bytes; a cloud searched without an index has its records in row order and needs none).
__global__ void __launch_bounds__(256) row_pos_kernel(const pcr_pt* __restrict__ pts, long long n, unsigned int* __restrict__ row_pos) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) row_pos[pts[j].id] = (unsigned int)j;
}

__global__ void __launch_bounds__(64)
fpfh_rows_lists_kernel(pcr_grid_view gv, long long n, const unsigned int* __restrict__ row_pos /* null: position = row */, double r2, int max_nn,
                       const long long* __restrict__ rows, long long m, unsigned int* __restrict__ need /* (n), zeroed */, unsigned int* __restrict__ nb_id /* (m,max_nn) */,
                       double* __restrict__ nb_d2, int* __restrict__ nb_cnt /* (m) */, int* __restrict__ fail) {
    __shared__ hybrid_lds s_L;
    const long long i = blockIdx.x;
    if (i >= m) return;
    const long long row = rows[i];
    if (row < 0 || row >= n) { if (threadIdx.x == 0) nb_cnt[i] = 0; return; }   // (the entry point refuses such rows; a resident caller gets zeros)
    const pcr_pt p = gv.pts[row_pos ? (long long)row_pos[row] : row];
    const int cnt = gather_hybrid<NB_CAP>(gv, p.x, p.y, p.z, r2, max_nn, &s_L);
    if (cnt < 0) { if (threadIdx.x == 0) { atomicAdd(fail, 1); nb_cnt[i] = 0; } return; }   // (as spfh_body: an empty list for the launch behind)
    for (int k = threadIdx.x; k < cnt; k += 64) {
        const nb_entry en = s_L.nb[k];
        nb_id[i * max_nn + k] = en.id;
        nb_d2[i * max_nn + k] = en.d2;
        need[en.id] = 1u;
    }
    if (threadIdx.x == 0) { nb_cnt[i] = cnt; need[row] = 1u; }
}

__global__ void __launch_bounds__(64)
spfh_rows_kernel(pcr_grid_view gv, const unsigned int* __restrict__ row_pos, double r2, int max_nn, const double* __restrict__ normals /* by row */,
                 const unsigned int* __restrict__ marked, const unsigned int* __restrict__ n_marked, unsigned int* __restrict__ slot /* (n): was `need` */,
                 double* __restrict__ spfh /* (bound,33) */, int* __restrict__ fail) {
    __shared__ hybrid_lds s_L;
    __shared__ int hist[33];
    const unsigned int k = blockIdx.x;
    if (k >= *n_marked) return;
    const unsigned int row = marked[k];
    if (threadIdx.x == 0) slot[row] = k;
    const pcr_pt p = gv.pts[row_pos ? row_pos[row] : row];
    spfh_body<NB_CAP, false>(gv, p, r2, max_nn, normals, spfh_dest{spfh + 33 * (size_t)k, nullptr, nullptr, nullptr}, fail, &s_L, hist);
}

__global__ void __launch_bounds__(64)
fpfh_rows_kernel(long long n, long long m, int max_nn, const long long* __restrict__ rows, const double* __restrict__ spfh, const unsigned int* __restrict__ slot,
                 const unsigned int* __restrict__ nb_id, const double* __restrict__ nb_d2, const int* __restrict__ nb_cnt, double* __restrict__ fpfh /* (m,33) */) {
    __shared__ unsigned int s_id[NB_CAP];
    __shared__ double s_d2[NB_CAP];
    __shared__ double s_acc[33];
    const long long i = blockIdx.x;
    if (i >= m) return;
    const long long row = rows[i];
    if (row < 0 || row >= n) { if (threadIdx.x < 33) fpfh[33 * i + threadIdx.x] = 0.0; return; }
    fpfh_body<true>(i, (long long)slot[row], max_nn, spfh, slot, nb_id, nb_d2, nb_cnt, fpfh + 33 * i, s_id, s_d2, s_acc);
}

// ------------------------------------------------------------------ host side
namespace {
int* fail_word(pcr_ctx* ctx) { return (int*)pcr_counter(ctx, PCR_CW_FEATURES_FAIL); }

// A cloud of a few thousand points (what the 2 m down-sample of main.py:35 leaves of a scan: 300 - 1 500 points) is searched without
// an index: two grid builds per scan -- one per radius, ~20 launches each -- cost several times what the neighbourhoods themselves
// cost, and a wave reads 4 096 records in 64 trips.  The "view" of such a cloud: its records in row order, levels = 0.
bool brute_view(const pcr_cloud* cloud, pcr_grid_view* v) {
    if (cloud->n > HYBRID_BRUTE_MAX || cloud->morton_sorted) return false;
    memset(v, 0, sizeof(*v));
    v->pts = cloud->d; v->n = cloud->n;
    v->levels = 0; v->cell0 = 1.0; v->inv_cell0 = 1.0;
    return true;
}

// Where a cloud's hybrid neighbourhoods are searched: the cloud itself (brute_view), else a grid index with cell >= radius, which goes
// back to the context when this leaves scope -- behind the caller's launches (stream-ordered).
struct hybrid_space {
    pcr_ctx* ctx; pcr_index* idx = nullptr; pcr_grid_view view;
    explicit hybrid_space(pcr_ctx* c) : ctx(c) {}
    ~hybrid_space() { if (idx) pcr_index_free(ctx, idx); }
    int open(const pcr_cloud* cloud, double radius) {
        if (brute_view(cloud, &view)) return PCR_OK;
        const int rc = pcr_index_build(ctx, cloud, PCR_INDEX_GRID, radius, &idx);
        if (rc) return rc;
        if (!(idx->view.cell0 >= radius)) { ctx->last_error = "radius too small for the cloud's extent"; return PCR_E_UNSUPPORTED; }
        view = idx->view;
        return PCR_OK;
    }
};

int launch_status(pcr_ctx* ctx) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { ctx->last_error = hipGetErrorString(e); return PCR_E_HIP; }
    return PCR_OK;
}
}  // namespace

int pcr_read_fail(pcr_ctx* ctx) {
    int fail = 0;
    const int rc = pcr_d2h_small(ctx, &fail, fail_word(ctx), sizeof(int));   // (synchronises)
    if (rc) return rc;
    if (fail) { hipMemsetAsync(fail_word(ctx), 0, sizeof(int), ctx->stream); ctx->last_error = "more than 1024 equidistant neighbours"; return PCR_E_UNSUPPORTED; }
    return PCR_OK;
}

int pcr_hybrid_normals_device(pcr_ctx* ctx, const pcr_cloud* cloud, double radius, int max_nn, int orient, const double* viewpoint, double* d_normals) {
    hybrid_space sp(ctx);
    const int rc = sp.open(cloud, radius);
    if (rc) return rc;
    const double v[3] = {viewpoint ? viewpoint[0] : 0.0, viewpoint ? viewpoint[1] : 0.0, viewpoint ? viewpoint[2] : 0.0};
    hipLaunchKernelGGL(hybrid_normals_kernel, dim3((unsigned)cloud->n), dim3(64), 0, ctx->stream, sp.view, (long long)cloud->n, radius * radius, max_nn,
                       orient, v[0], v[1], v[2], d_normals, fail_word(ctx));
    return launch_status(ctx);
}

int pcr_fpfh_device(pcr_ctx* ctx, const pcr_cloud* cloud, const double* d_normals, double radius, int max_nn, double* d_out) {
    const long long n = cloud->n;
    pcr_dev_block spfh(ctx), nbid(ctx), nbd2(ctx), nbcnt(ctx);
    int rc;
    if ((rc = spfh.alloc(sizeof(double) * 33 * n)) || (rc = nbid.alloc(sizeof(unsigned int) * (size_t)max_nn * n)) || (rc = nbd2.alloc(sizeof(double) * (size_t)max_nn * n)) ||
        (rc = nbcnt.alloc(sizeof(int) * n)))
        return rc;
    hybrid_space sp(ctx);
    if ((rc = sp.open(cloud, radius))) return rc;
    hipLaunchKernelGGL(spfh_kernel, dim3((unsigned)n), dim3(64), 0, ctx->stream, sp.view, n, radius * radius, max_nn, d_normals,
                       spfh.as<double>(), nbid.as<unsigned int>(), nbd2.as<double>(), nbcnt.as<int>(), fail_word(ctx));
    hipLaunchKernelGGL(fpfh_kernel, dim3((unsigned)n), dim3(64), 0, ctx->stream, n, max_nn, (const double*)spfh.as<double>(),
                       (const unsigned int*)nbid.as<unsigned int>(), (const double*)nbd2.as<double>(), (const int*)nbcnt.as<int>(), d_out);
    return launch_status(ctx);   // (the index and the scratch go back to the arena stream-ordered)
}

// Scratch: 12 m max_nn + 4 m for the lists, 4 n (8 n with the position table) for need / slot, 268 bytes per row of the bound for the
// marked rows and their SPFH -- against n (12 max_nn + 268) of the full pass.
int pcr_fpfh_rows_device(pcr_ctx* ctx, const pcr_cloud* cloud, const double* d_normals, double radius, int max_nn, const long long* d_rows, long long m, double* d_out,
                         unsigned int* d_n_spfh) {
    const long long n = cloud->n;
    if (m <= 0) { PCR_HIP(ctx, hipMemsetAsync(d_n_spfh, 0, sizeof(unsigned int), ctx->stream)); return PCR_OK; }
    const long long bound = m <= n / (max_nn + 1) ? m * (max_nn + 1) : n;   // >= the marked rows, whatever they turn out to be
    pcr_dev_block need(ctx), rowpos(ctx), marked(ctx), spfh(ctx), nbid(ctx), nbd2(ctx), nbcnt(ctx), tmp(ctx);
    int rc;
    if (m > 0x7fffffffLL) return PCR_E_INVALID;   // (one block per entry)
    if ((rc = need.alloc(sizeof(unsigned int) * n)) || (rc = marked.alloc(sizeof(unsigned int) * bound)) ||
        (rc = spfh.alloc(sizeof(double) * 33 * bound)) || (rc = nbid.alloc(sizeof(unsigned int) * (size_t)max_nn * m)) || (rc = nbd2.alloc(sizeof(double) * (size_t)max_nn * m)) ||
        (rc = nbcnt.alloc(sizeof(int) * m)))
        return rc;
    hybrid_space sp(ctx);
    if ((rc = sp.open(cloud, radius))) return rc;
    const bool table = sp.idx != nullptr;   // (an index's records are in its own order; brute_view's are in row order)
    if (table && (rc = rowpos.alloc(sizeof(unsigned int) * n))) return rc;
    PCR_HIP(ctx, hipMemsetAsync(need.p, 0, sizeof(unsigned int) * n, ctx->stream));
    if (table) hipLaunchKernelGGL(row_pos_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, sp.view.pts, n, rowpos.as<unsigned int>());
    const unsigned int* const pos = table ? rowpos.as<unsigned int>() : nullptr;
    hipLaunchKernelGGL(fpfh_rows_lists_kernel, dim3((unsigned)m), dim3(64), 0, ctx->stream, sp.view, n, pos, radius * radius, max_nn, d_rows, m, need.as<unsigned int>(),
                       nbid.as<unsigned int>(), nbd2.as<double>(), nbcnt.as<int>(), fail_word(ctx));
    if ((rc = pcr_select_positions(ctx, need.as<unsigned int>(), (size_t)n, marked.as<unsigned int>(), d_n_spfh, tmp))) return rc;
    hipLaunchKernelGGL(spfh_rows_kernel, dim3((unsigned)bound), dim3(64), 0, ctx->stream, sp.view, pos, radius * radius, max_nn, d_normals, (const unsigned int*)marked.as<unsigned int>(),
                       (const unsigned int*)d_n_spfh, need.as<unsigned int>(), spfh.as<double>(), fail_word(ctx));
    hipLaunchKernelGGL(fpfh_rows_kernel, dim3((unsigned)m), dim3(64), 0, ctx->stream, n, m, max_nn, d_rows, (const double*)spfh.as<double>(), (const unsigned int*)need.as<unsigned int>(),
                       (const unsigned int*)nbid.as<unsigned int>(), (const double*)nbd2.as<double>(), (const int*)nbcnt.as<int>(), d_out);
    return launch_status(ctx);   // (the index and the scratch go back to the arena stream-ordered)
}

int pcr_scans_features(pcr_ctx* ctx, const scans_view& V, size_t ng, const pcr_global_params* g, const scans_scratch& w, double* d_fpfh) {
    unsigned int* const redo_n = pcr_counter(ctx, PCR_CW_FEATURES_REDO);   // [0]: normals, [1]: SPFH (zero between calls)
    const unsigned fixed = (unsigned)(ng < (size_t)(16 * ctx->cu_count) ? ng : (size_t)(16 * ctx->cu_count));
    const unsigned int* const none = nullptr;
    if (hipMemsetAsync(redo_n, 0, 8, ctx->stream) != hipSuccess) return PCR_E_HIP;
    hipLaunchKernelGGL(normals_scans_kernel<128>, dim3((unsigned)ng), dim3(64), 0, ctx->stream, V, (long long)ng, g->normal_radius * g->normal_radius, g->normal_max_nn,
                       w.normals, fail_word(ctx), none, none, w.redo, redo_n, w.cov);
    hipLaunchKernelGGL(normals_scans_kernel<NB_CAP>, dim3(fixed), dim3(64), 0, ctx->stream, V, (long long)ng, g->normal_radius * g->normal_radius, g->normal_max_nn,
                       w.normals, fail_word(ctx), (const unsigned int*)w.redo, (const unsigned int*)redo_n, (unsigned int*)nullptr, (unsigned int*)nullptr, w.cov);
    hipLaunchKernelGGL(normals_finish_kernel, dim3((unsigned)((ng + 255) / 256)), dim3(256), 0, ctx->stream, V, (long long)ng, (const double*)w.cov, w.normals);
    // (the SPFH list is written behind the normals' one: both launches of a stage are done before the next stage's first)
    hipLaunchKernelGGL(spfh_scans_kernel<256>, dim3((unsigned)ng), dim3(64), 0, ctx->stream, V, (long long)ng, g->fpfh_radius * g->fpfh_radius, g->fpfh_max_nn,
                       (const double*)w.normals, w.spfh, w.nb_id, w.nb_d2, w.nb_cnt, fail_word(ctx), none, none, w.redo, redo_n + 1);
    hipLaunchKernelGGL(spfh_scans_kernel<NB_CAP>, dim3(fixed), dim3(64), 0, ctx->stream, V, (long long)ng, g->fpfh_radius * g->fpfh_radius, g->fpfh_max_nn,
                       (const double*)w.normals, w.spfh, w.nb_id, w.nb_d2, w.nb_cnt, fail_word(ctx), (const unsigned int*)w.redo, (const unsigned int*)(redo_n + 1),
                       (unsigned int*)nullptr, (unsigned int*)nullptr);
    const auto fpfh_k = g->fpfh_max_nn <= 128 ? fpfh_scans_kernel<128> : fpfh_scans_kernel<NB_CAP>;   // (LDS for the longest list)
    hipLaunchKernelGGL(fpfh_k, dim3((unsigned)ng), dim3(64), 0, ctx->stream, V, (long long)ng, g->fpfh_max_nn, (const double*)w.spfh, (const unsigned int*)w.nb_id,
                       (const double*)w.nb_d2, (const int*)w.nb_cnt, d_fpfh);
    return PCR_OK;
}

extern "C" {
int pcr_normals_hybrid(pcr_ctx* ctx, const pcr_cloud* cloud, double radius, int max_nn, int orient, const double viewpoint[3], double* normals_out) {
    if (!ctx || !cloud || !normals_out || !hybrid_params_ok(radius, max_nn, 1)) return PCR_E_INVALID;
    if (cloud->n <= 0) return PCR_E_EMPTY;
    hipSetDevice(ctx->device);
    pcr_dev_block nrm(ctx);
    int rc;
    if ((rc = nrm.alloc(sizeof(double) * 3 * cloud->n)) || (rc = pcr_hybrid_normals_device(ctx, cloud, radius, max_nn, orient, viewpoint, nrm.as<double>()))) return rc;
    PCR_HIP(ctx, hipMemcpyAsync(normals_out, nrm.p, sizeof(double) * 3 * cloud->n, hipMemcpyDeviceToHost, ctx->stream));
    return pcr_read_fail(ctx);
}

int pcr_fpfh(pcr_ctx* ctx, const pcr_cloud* cloud, const double* normals, double radius, int max_nn, double* features_out) {
    if (!ctx || !cloud || !normals || !features_out || !hybrid_params_ok(radius, max_nn, 2)) return PCR_E_INVALID;
    if (cloud->n <= 0) return PCR_E_EMPTY;
    hipSetDevice(ctx->device);
    const long long n = cloud->n;
    pcr_dev_block nrm(ctx), out(ctx);
    int rc;
    if ((rc = nrm.alloc(sizeof(double) * 3 * n)) || (rc = out.alloc(sizeof(double) * 33 * n))) return rc;
    PCR_HIP(ctx, hipMemcpyAsync(nrm.p, normals, sizeof(double) * 3 * n, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = pcr_fpfh_device(ctx, cloud, nrm.as<double>(), radius, max_nn, out.as<double>()))) return rc;
    PCR_HIP(ctx, hipMemcpyAsync(features_out, out.p, sizeof(double) * 33 * n, hipMemcpyDeviceToHost, ctx->stream));
    return pcr_read_fail(ctx);
}

int pcr_fpfh_rows(pcr_ctx* ctx, const pcr_cloud* cloud, const double* normals, double radius, int max_nn, const int64_t* rows, int64_t m, double* features_out,
                  int64_t* n_spfh_out) {
    if (!ctx || !cloud || !normals || !rows || !features_out || m < 0 || !hybrid_params_ok(radius, max_nn, 2)) return PCR_E_INVALID;
    if (cloud->n <= 0) return PCR_E_EMPTY;
    const long long n = cloud->n;
    for (int64_t i = 0; i < m; ++i)
        if (rows[i] < 0 || rows[i] >= n) return PCR_E_INVALID;
    if (m == 0) { if (n_spfh_out) *n_spfh_out = 0; return PCR_OK; }
    static_assert(sizeof(long long) == sizeof(int64_t), "rows are uploaded as they are");
    hipSetDevice(ctx->device);
    pcr_dev_block nrm(ctx), d_rows(ctx), out(ctx), count(ctx);
    int rc;
    if ((rc = nrm.alloc(sizeof(double) * 3 * n)) || (rc = d_rows.alloc(sizeof(long long) * m)) || (rc = out.alloc(sizeof(double) * 33 * m)) || (rc = count.alloc(16))) return rc;
    PCR_HIP(ctx, hipMemcpyAsync(nrm.p, normals, sizeof(double) * 3 * n, hipMemcpyHostToDevice, ctx->stream));
    PCR_HIP(ctx, hipMemcpyAsync(d_rows.p, rows, sizeof(long long) * m, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = pcr_fpfh_rows_device(ctx, cloud, nrm.as<double>(), radius, max_nn, d_rows.as<long long>(), m, out.as<double>(), count.as<unsigned int>()))) return rc;
    unsigned int n_spfh = 0;
    PCR_HIP(ctx, hipMemcpyAsync(features_out, out.p, sizeof(double) * 33 * m, hipMemcpyDeviceToHost, ctx->stream));
    PCR_HIP(ctx, hipMemcpyAsync(&n_spfh, count.p, sizeof(unsigned int), hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = pcr_read_fail(ctx))) return rc;   // (the one wait of the call: both copies are done behind it)
    if (n_spfh_out) *n_spfh_out = (int64_t)n_spfh;
    return PCR_OK;
}
}  // extern "C"
