// RANSAC of the global initialisation (stages: pcr_global_dev.h):
//   pcr_ransac           3-point RANSAC with edge-length and distance checkers   Registration/main.py:73-83, icp_template.py:88-110
// for one pair (ransac_kernel / ransac_walk_kernel) and for every pair of a share at once (the _jobs kernels).
#include <cfloat>
#include <cmath>
#include <cstring>
#include "pcr_grid_dev.h"
#include "pcr_linalg.h"
#include "pcr_global_dev.h"

// --------------------------------------------------------------------- RANSAC
// The loop of registration_ransac_based_on_feature_matching (main.py:73-83) / ransac_init (icp_template.py:88-110) stays on the
// device: a batch of hypotheses is evaluated side by side (one wave each), then ONE wave walks the batch in iteration order --
// running best, confidence-based exit -- exactly as the sequential loop would, and leaves the loop state in device memory; the
// batches behind a stop return at once.  The host enqueues every batch and synchronises once.
struct ransac_args {
    const pcr_pt* src;  // by row (id == position)
    const pcr_pt* tgt;
    const int* corr;    // (m,2)
    int first_iter, n_iter;
    unsigned long long seed;
    double edge_sim;    // <= 0: checker off
    double max_dist;    // inlier threshold and distance checker
    int check_distance;
    int max_iteration;
    double confidence;
};

__host__ __device__ static inline ransac_args ransac_make_args(const pcr_pt* src, const pcr_pt* tgt, const int* corr, unsigned long long seed, const ransac_common& c) {
    return ransac_args{src, tgt, corr, c.first_iter, c.n_iter, seed, c.edge_sim, c.max_dist, c.check_distance, c.max_iteration, c.confidence};
}

__host__ __device__ static inline unsigned long long mix64(unsigned long long x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// out: inl[h] (-1 = rejected by a checker), err2[h], T[h][12]
// 64 hypotheses per wave: every LANE draws its own sample and runs the checkers and the Kabsch step on it (the same scalar code the whole
// wave used to run 64 times over for one hypothesis); the few that pass are then scored one after the other by all 64 lanes together.
// Same arithmetic per hypothesis as ever: the batch's results do not depend on how hypotheses are dealt to waves.
__device__ static void ransac_eval(const ransac_args& a, const ransac_state* __restrict__ st, int* __restrict__ inl, double* __restrict__ err2,
                                   double* __restrict__ Tout, const int h_base) {
    if (h_base >= a.n_iter || st->stop) return;
    const int lane = threadIdx.x;
    const int h = h_base + lane;
    const int m = st->m;
    const unsigned long long itr = (unsigned long long)(a.first_iter + h);
    // (a hypothesis at or behind exit_itr is never looked at by the walk)
    const bool mine = h < a.n_iter && (long long)itr < st->exit_itr;
    bool ok = mine;
    double R[9], tr[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = 0.0;
    tr[0] = tr[1] = tr[2] = 0.0;
    if (mine) {
        double s[3][3], t[3][3];
        for (int j = 0; j < 3; ++j) {
            const unsigned int c = (unsigned int)(mix64(a.seed ^ mix64(itr * 3 + j)) % (unsigned long long)m);
            const pcr_pt ps = a.src[a.corr[2 * c]], pt = a.tgt[a.corr[2 * c + 1]];
            s[j][0] = ps.x; s[j][1] = ps.y; s[j][2] = ps.z;
            t[j][0] = pt.x; t[j][1] = pt.y; t[j][2] = pt.z;
        }
        if (a.edge_sim > 0) {
            for (int i = 0; i < 3 && ok; ++i)
                for (int j = i + 1; j < 3; ++j) {
                    const double ds = sqrt(((s[i][0] - s[j][0]) * (s[i][0] - s[j][0]) + (s[i][1] - s[j][1]) * (s[i][1] - s[j][1])) + (s[i][2] - s[j][2]) * (s[i][2] - s[j][2]));
                    const double dt = sqrt(((t[i][0] - t[j][0]) * (t[i][0] - t[j][0]) + (t[i][1] - t[j][1]) * (t[i][1] - t[j][1])) + (t[i][2] - t[j][2]) * (t[i][2] - t[j][2]));
                    if (ds < dt * a.edge_sim || dt < ds * a.edge_sim) { ok = false; break; }
                }
        }
        if (ok) {
            // Kabsch on the three pairs (procrustes_transformation, icp_template.py:43-54; proper rotation for the rank-2 case)
            double mo[18];
            for (int k = 0; k < 18; ++k) mo[k] = 0.0;
            const double org[3] = {s[0][0], s[0][1], s[0][2]};
            mo[0] = 3.0;
            for (int j = 0; j < 3; ++j) {
                const double ax = s[j][0] - org[0], ay = s[j][1] - org[1], az = s[j][2] - org[2];
                const double bx = t[j][0] - org[0], by = t[j][1] - org[1], bz = t[j][2] - org[2];
                mo[1] += ax; mo[2] += ay; mo[3] += az;
                mo[4] += bx; mo[5] += by; mo[6] += bz;
                mo[7] += bx * ax; mo[8] += bx * ay; mo[9] += bx * az;
                mo[10] += by * ax; mo[11] += by * ay; mo[12] += by * az;
                mo[13] += bz * ax; mo[14] += bz * ay; mo[15] += bz * az;
                mo[16] += (ax * ax + ay * ay) + az * az;
                mo[17] += (bx * bx + by * by) + bz * bz;
            }
            pcr::kabsch_from_moments(mo, org, R, tr, nullptr);
            for (int k = 0; k < 9; ++k) ok = ok && (R[k] == R[k]);
            if (ok && a.check_distance) {
                for (int j = 0; j < 3; ++j) {
                    const double x = ((R[0] * s[j][0] + R[1] * s[j][1]) + R[2] * s[j][2]) + tr[0] - t[j][0];
                    const double y = ((R[3] * s[j][0] + R[4] * s[j][1]) + R[5] * s[j][2]) + tr[1] - t[j][1];
                    const double z = ((R[6] * s[j][0] + R[7] * s[j][1]) + R[8] * s[j][2]) + tr[2] - t[j][2];
                    if (sqrt((x * x + y * y) + z * z) > a.max_dist) ok = false;
                }
            }
        }
        if (!ok) { inl[h] = -1; err2[h] = 0.0; }
    }
    // ---- the survivors, one after the other, scored by the whole wave
    unsigned long long mk = __ballot(ok);
    while (mk) {
        const int l = (int)__ffsll((long long)mk) - 1;
        mk &= mk - 1;
        double Rl[9], tl[3];
#pragma unroll
        for (int k = 0; k < 9; ++k) Rl[k] = __shfl(R[k], l, 64);
#pragma unroll
        for (int k = 0; k < 3; ++k) tl[k] = __shfl(tr[k], l, 64);
        int good = 0;
        double e2 = 0.0;
        for (int c = lane; c < m; c += 64) {
            const pcr_pt ps = a.src[a.corr[2 * c]], pt = a.tgt[a.corr[2 * c + 1]];
            const double x = ((Rl[0] * ps.x + Rl[1] * ps.y) + Rl[2] * ps.z) + tl[0] - pt.x;
            const double y = ((Rl[3] * ps.x + Rl[4] * ps.y) + Rl[5] * ps.z) + tl[1] - pt.y;
            const double z = ((Rl[6] * ps.x + Rl[7] * ps.y) + Rl[8] * ps.z) + tl[2] - pt.z;
            const double dis = sqrt((x * x + y * y) + z * z);
            if (dis < a.max_dist) { ++good; e2 += dis * dis; }
        }
        e2 = wave_sum_all(e2);
        good = wave_sum_all(good);
        if (lane == 0) {
            const int hl = h_base + l;
            inl[hl] = good;
            err2[hl] = e2;
            for (int k = 0; k < 9; ++k) Tout[12 * (long long)hl + k] = Rl[k];
            for (int k = 0; k < 3; ++k) Tout[12 * (long long)hl + 9 + k] = tl[k];
        }
    }
}

__global__ void __launch_bounds__(64) ransac_kernel(ransac_args a, const ransac_state* __restrict__ st, int* __restrict__ inl, double* __restrict__ err2,
                                                    double* __restrict__ Tout) {
    ransac_eval(a, st, inl, err2, Tout, 64 * (int)blockIdx.x);
}

// ONE wave: the sequential loop over the batch -- iteration order, running best (IsBetterRANSACThan: higher fitness, or equal
// fitness and lower rmse; the initial best is (0, 0)), exit_itr = min(exit_itr, ceil(log(1 - confidence) / log(1 - fitness^3)))
// after every improvement, stop at the first iteration >= exit_itr -- 64 iterations at a time: inside a chunk the NEXT improvement
// is the first lane that beats the current best (the order is a strict weak order, so nobody in front of it can beat the new best).
__device__ static void ransac_walk(const ransac_args& a, ransac_state* __restrict__ st, const int* __restrict__ inl, const double* __restrict__ err2,
                                   const double* __restrict__ Tout) {
    if (st->stop) return;
    const int lane = threadIdx.x;
    const int m = st->m;
    double best_fit = st->best_fit, best_rmse = st->best_rmse;
    long long best_itr = st->best_itr, exit_itr = st->exit_itr, n_valid = st->n_valid;
    int best_h = -1;
    bool stop = false;
    for (int base = 0; base < a.n_iter && !stop; base += 64) {
        const int h = base + lane;
        const long long itr = (long long)a.first_iter + h;
        bool active = h < a.n_iter && itr < exit_itr;
        int good = -1;
        double e2 = 0.0;
        if (active) { good = inl[h]; e2 = err2[h]; }
        const bool valid = good >= 0;
        const double fit = valid ? (double)good / (double)m : 0.0;
        const double rmse = good > 0 ? sqrt(e2 / (double)good) : 0.0;
        for (;;) {
            const bool cand = active && valid && (fit > best_fit || (fit == best_fit && rmse < best_rmse));
            const unsigned long long mk = __ballot(cand);
            if (!mk) break;
            const int l = (int)__ffsll((long long)mk) - 1;
            best_fit = __shfl(fit, l, 64);
            best_rmse = __shfl(rmse, l, 64);
            best_itr = (long long)a.first_iter + base + l;
            best_h = base + l;
            const double x = 1.0 - pow(best_fit, 3.0);
            const double k = x <= 0.0 ? 0.0 : log(1.0 - a.confidence) / log(x);
            if (k < (double)a.max_iteration) { const long long ke = (long long)ceil(k); if (ke < exit_itr) exit_itr = ke; }
            if (lane > l) active = active && itr < exit_itr;   // what comes after the improvement sees the new exit
        }
        n_valid += __popcll(__ballot(active && valid));
        if ((long long)a.first_iter + base + 64 >= exit_itr) stop = true;   // the next chunk starts at or behind exit_itr
    }
    const long long end = (long long)a.first_iter + a.n_iter;
    if (best_h >= 0 && lane < 12) st->bestT[lane] = Tout[12 * (long long)best_h + lane];
    if (lane == 0) {
        st->best_fit = best_fit; st->best_rmse = best_rmse; st->best_itr = best_itr; st->exit_itr = exit_itr; st->n_valid = n_valid;
        st->done = end < exit_itr ? end : exit_itr;
        if (end >= exit_itr) st->stop = 1;
    }
}

__global__ void __launch_bounds__(64) ransac_walk_kernel(ransac_args a, ransac_state* __restrict__ st, const int* __restrict__ inl, const double* __restrict__ err2,
                                                         const double* __restrict__ Tout) {
    ransac_walk(a, st, inl, err2, Tout);
}

__global__ void ransac_init_kernel(ransac_state* st, const int* m_p, int max_iteration) { ransac_init(st, m_p, max_iteration); }

// active: the jobs still running (indices into jobs), or null = all
__global__ void __launch_bounds__(64) ransac_jobs_kernel(const init_job* __restrict__ jobs, const int* __restrict__ active, ransac_common c) {
    const init_job J = jobs[active ? active[blockIdx.y] : blockIdx.y];
    const ransac_args a = ransac_make_args(J.src, J.tgt, J.corr, J.seed, c);
    ransac_eval(a, J.st, J.inl, J.err2, J.Tout, 64 * (int)blockIdx.x);
}
__global__ void __launch_bounds__(64) ransac_walk_jobs_kernel(const init_job* __restrict__ jobs, const int* __restrict__ active, ransac_common c) {
    const init_job J = jobs[active ? active[blockIdx.x] : blockIdx.x];
    const ransac_args a = ransac_make_args(J.src, J.tgt, J.corr, J.seed, c);
    ransac_walk(a, J.st, J.inl, J.err2, J.Tout);
}

// ------------------------------------------------------------------ host side
int pcr_ransac_device(pcr_ctx* ctx, const pcr_pt* d_src, const pcr_pt* d_tgt, const int* d_corr, const int* d_m, const pcr_ransac_params* prm, pcr_ransac_result* res) {
    memset(res, 0, sizeof(*res));
    for (int k = 0; k < 4; ++k) res->T[5 * k] = 1.0;
    pcr_dev_block dinl(ctx), derr(ctx), dT(ctx), dst(ctx);
    int rc;
    if ((rc = dinl.alloc(sizeof(int) * RANSAC_BATCH)) || (rc = derr.alloc(sizeof(double) * RANSAC_BATCH)) || (rc = dT.alloc(sizeof(double) * 12 * RANSAC_BATCH)) ||
        (rc = dst.alloc(sizeof(ransac_state))))
        return rc;
    ransac_state* const st = dst.as<ransac_state>();
    hipLaunchKernelGGL(ransac_init_kernel, dim3(1), dim3(64), 0, ctx->stream, st, d_m, prm->max_iteration);
    ransac_common c = ransac_common_of(prm);
    // the first two batches (20 480 iterations) go out together -- most registrations exit within the first thousand --, then
    // the state is looked at; what is left of the budget follows in one go (batches behind a stop return at once)
    ransac_state h;
    long long done = 0;
    for (int round = 0; done < prm->max_iteration; ++round) {
        for (int b = 0; done < prm->max_iteration && (round > 0 || b < 2); ++b) {
            const int nb = ransac_batch_size(done, prm->max_iteration);
            c.first_iter = (int)done; c.n_iter = nb;
            const ransac_args a = ransac_make_args(d_src, d_tgt, d_corr, prm->seed, c);
            hipLaunchKernelGGL(ransac_kernel, dim3((nb + 63) / 64), dim3(64), 0, ctx->stream, a, (const ransac_state*)st, dinl.as<int>(), derr.as<double>(), dT.as<double>());
            hipLaunchKernelGGL(ransac_walk_kernel, dim3(1), dim3(64), 0, ctx->stream, a, st, (const int*)dinl.as<int>(), (const double*)derr.as<double>(), (const double*)dT.as<double>());
            done += nb;
        }
        PCR_HIP(ctx, hipGetLastError());
        if ((rc = pcr_d2h_small(ctx, &h, st, sizeof(h)))) return rc;   // (synchronises)
        if (h.stop) break;
    }
    if (h.m < 3) return PCR_E_TOO_FEW_ASSOC;
    res->iterations = (int)h.done; res->n_valid = (int)h.n_valid; res->best_iteration = (int)h.best_itr;
    res->corr_fitness = h.best_fit; res->corr_rmse = h.best_rmse;
    res->reserved_i = h.m;   // size of the correspondence set that was sampled
    if (h.best_itr < 0) return PCR_E_TOO_FEW_ASSOC;  // no hypothesis passed the checkers: identity
    ransac_T16(h.bestT, res->T);
    return PCR_OK;
}

void pcr_ransac_jobs_round(pcr_ctx* ctx, const init_job* d_jobs, const int* d_active, int n_run, const ransac_common& c) {
    hipLaunchKernelGGL(ransac_jobs_kernel, dim3((c.n_iter + 63) / 64, n_run), dim3(64), 0, ctx->stream, d_jobs, d_active, c);
    hipLaunchKernelGGL(ransac_walk_jobs_kernel, dim3(n_run), dim3(64), 0, ctx->stream, d_jobs, d_active, c);
}

extern "C" {
int pcr_ransac_default_params(pcr_ransac_params* p) {
    if (!p) return PCR_E_INVALID;
    memset(p, 0, sizeof(*p));
    p->max_iteration = 100000;   // RANSACConvergenceCriteria(100000, 0.999), main.py:83
    p->confidence = 0.999;
    p->max_distance = 3.0;       // voxel_size * 1.5 with voxel_size = 2.0, main.py:70,197
    p->edge_similarity = 0.9;    // CorrespondenceCheckerBasedOnEdgeLength(0.9), main.py:78-79
    p->check_distance = 1;       // CorrespondenceCheckerBasedOnDistance, main.py:80-81
    p->seed = 0;
    return PCR_OK;
}

int pcr_ransac(pcr_ctx* ctx, const pcr_cloud* source, const pcr_cloud* target, const int32_t* corr, int64_t m, const pcr_ransac_params* prm,
               pcr_ransac_result* res) {
    if (!ctx || !source || !target || !corr || !res || !ransac_params_ok(prm)) return PCR_E_INVALID;
    memset(res, 0, sizeof(*res));
    for (int k = 0; k < 4; ++k) res->T[5 * k] = 1.0;
    if (m < 3) return PCR_E_TOO_FEW_ASSOC;
    if (m > 0x7fffffffll) return PCR_E_UNSUPPORTED;
    for (int64_t c = 0; c < m; ++c)
        if (corr[2 * c] < 0 || corr[2 * c] >= source->n || corr[2 * c + 1] < 0 || corr[2 * c + 1] >= target->n) return PCR_E_INVALID;
    hipSetDevice(ctx->device);
    // clouds in caller row order
    pcr_dev_block s(ctx), t(ctx), dc(ctx);
    int rc;
    if ((rc = s.alloc(sizeof(pcr_pt) * source->n)) || (rc = t.alloc(sizeof(pcr_pt) * target->n)) || (rc = dc.alloc(sizeof(int) * 2 * m + 16))) return rc;
    if ((rc = pcr_cloud_rows(ctx, source, s.as<pcr_pt>())) || (rc = pcr_cloud_rows(ctx, target, t.as<pcr_pt>()))) return rc;
    const int m32 = (int)m;
    PCR_HIP(ctx, hipMemcpyAsync(dc.p, corr, sizeof(int) * 2 * m, hipMemcpyHostToDevice, ctx->stream));
    PCR_HIP(ctx, hipMemcpyAsync(dc.as<int>() + 2 * m, &m32, sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    return pcr_ransac_device(ctx, s.as<pcr_pt>(), t.as<pcr_pt>(), dc.as<int>(), dc.as<int>() + 2 * m, prm, res);
}
}  // extern "C"
