// What the stages of the global initialisation share (pcr_features.hip, pcr_match.hip, pcr_ransac.hip; sequenced by pcr_global_init.hip).
// The library has no relocatable device code: a kernel is launched only by the unit that defines it, and the units meet in HOST functions
// that enqueue on ctx->stream.  Nothing here synchronises unless it says so.
#pragma once
#include "pcr_wave.h"   // wave_sum_all

constexpr int NB_CAP = 1024;
// clouds of up to this many points are searched without an index (brute_view; the fused initialisation takes only such scans)
constexpr int HYBRID_BRUTE_MAX = 4096;
constexpr int JOB_SPLITS = 8, FM_STEPS = 9;   // FM_STEPS: 36 = 33 dimensions + the norm / one slot + 2 zeros
// RANSAC schedule: the first 4 096 iterations (most registrations exit within the first thousand), then 16 384 at a time
constexpr int RANSAC_FIRST = 4096, RANSAC_BATCH = 16384;
inline int ransac_batch_size(long long done, int max_iteration) {
    const long long want = done == 0 ? RANSAC_FIRST : RANSAC_BATCH, left = max_iteration - done;
    return (int)(left < want ? left : want);
}
// The down-sampled scans of a chunk, one behind the other (pcr_voxel_downsample_scans): record v belongs to scan vsid[v], whose records
// are [scan_first[s], scan_first[s + 1]) with id = row within the scan.  A block's "grid view" is its own scan, searched without an index.
struct scans_view { const pcr_pt* down; const unsigned int *vsid, *scan_first; };
// per-point scratch of a chunk's normals / SPFH / FPFH launches (ng points; lists of fpfh_max_nn)
struct scans_scratch {
    double *normals, *spfh;                             // (ng,3), (ng,33)
    unsigned int* nb_id; double* nb_d2; int* nb_cnt;    // (ng,max_nn) twice, (ng)
    unsigned int* redo;                                 // (ng): points left to the launch with the full candidate array
    double* cov;                                        // (ng,7)
};
struct ransac_state {
    double best_fit, best_rmse;
    double bestT[12];
    long long best_itr, exit_itr, done, n_valid;
    int stop, m;
    int pad[2];
};
__device__ static void ransac_init(ransac_state* st, const int* m_p, int max_iteration) {
    if (threadIdx.x != 0) return;
    ransac_state z;
    z.best_fit = 0.0; z.best_rmse = 0.0;
    for (int k = 0; k < 12; ++k) z.bestT[k] = 0.0;
    z.best_itr = -1; z.exit_itr = max_iteration; z.done = 0; z.n_valid = 0;
    z.m = *m_p;
    z.stop = z.m < 3 ? 1 : 0;
    z.pad[0] = z.pad[1] = 0;
    *st = z;
}
struct ransac_common { double edge_sim, max_dist, confidence; int check_distance, max_iteration, first_iter, n_iter; };
inline ransac_common ransac_common_of(const pcr_ransac_params* p) {   // (first_iter / n_iter: set per batch)
    return ransac_common{p->edge_similarity, p->max_distance, p->confidence, p->check_distance, p->max_iteration, 0, 0};
}
inline void ransac_T16(const double bestT[12] /* 3x3 | t */, double T[16] /* row-major 4x4 whose last row the caller has set */) {
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) T[4 * i + j] = bestT[3 * i + j];
        T[4 * i + 3] = bestT[9 + i];
    }
}

// ------------------------------------------------------------------------------------------------ every pair of a share at once
// The same stages with one launch for ALL pairs (a job = one pair; blockIdx.y / .z picks it): a pair alone is ten launches of a few
// microseconds of work each, and a share of the reference's pair loop (main.py:190-216) is hundreds of pairs.
struct init_job {
    const pcr_pt *src, *tgt;          // down-sampled records by row
    const double *fa, *fb;            // FPFH (n,33)
    int na, nb;
    int *ij, *ji;                     // nearest target row of every source row, and the other way
    double *dab, *dba;
    int *ci_ab, *ci_ba;               // per-split candidates (splits x n)
    double *cd_ab, *cd_ba;
    int *corr, *m;                    // (na,2) + count
    ransac_state* st;
    int* inl;                         // hypothesis scratch of a batch
    double *err2, *Tout;
    unsigned long long seed;
    // matrix-core operands of both descriptor sets (mfma_ops_kernel): as the sweep's targets, as its queries; squared norms; largest norm
    const double *ta, *tb, *qa, *qb, *n2a, *n2b, *mxa, *mxb;
    const unsigned int *mra, *mrb;    // row of the smallest norm (lowest row on ties) of either set: the answer for an all-zero query
};

// ---- argument checks shared by the entry points (false: PCR_E_INVALID)
inline bool hybrid_params_ok(double radius, int max_nn, int min_nn) { return radius > 0 && max_nn >= min_nn && max_nn <= NB_CAP; }
inline bool prep_params_ok(double voxel_size, double normal_radius, int normal_max_nn, double fpfh_radius, int fpfh_max_nn) {
    return voxel_size > 0 && hybrid_params_ok(normal_radius, normal_max_nn, 1) && hybrid_params_ok(fpfh_radius, fpfh_max_nn, 2);
}
inline bool ransac_params_ok(const pcr_ransac_params* p) { return p && p->max_iteration >= 1 && p->max_distance > 0; }

// ---- pcr_features.hip
// the context's fail word (a neighbourhood that could not be bounded bumps it): read, cleared, PCR_E_UNSUPPORTED if set.  Synchronises.
PCR_HIDDEN int pcr_read_fail(pcr_ctx* ctx);
// normals (n,3) / FPFH (n,33) of a device cloud, by row (a grid build inside synchronises once)
PCR_HIDDEN int pcr_hybrid_normals_device(pcr_ctx* ctx, const pcr_cloud* cloud, double radius, int max_nn, int orient, const double* viewpoint, double* d_normals);
PCR_HIDDEN int pcr_fpfh_device(pcr_ctx* ctx, const pcr_cloud* cloud, const double* d_normals, double radius, int max_nn, double* d_out);
// FPFH of the m caller rows d_rows (device; any order, repeats allowed) -> d_out (m,33): bit for bit those rows of pcr_fpfh_device's
// output, from the SPFH of the rows their lists reach only.  *d_n_spfh (device word, not null): how many rows that were.  Enqueued.
PCR_HIDDEN int pcr_fpfh_rows_device(pcr_ctx* ctx, const pcr_cloud* cloud, const double* d_normals, double radius, int max_nn, const long long* d_rows, long long m,
                                    double* d_out, unsigned int* d_n_spfh);
// normals (towards the origin), SPFH and FPFH of every down-sampled point of a chunk: d_fpfh (ng,33)
PCR_HIDDEN int pcr_scans_features(pcr_ctx* ctx, const scans_view& V, size_t ng, const pcr_global_params* g, const scans_scratch& w, double* d_fpfh);
// ---- pcr_match.hip
// nearest row of B (nb,dim) for every row of A (na,dim), both on the device
PCR_HIDDEN int pcr_feature_match_device(pcr_ctx* ctx, const double* dA, long long na, const double* dB, long long nb, int dim, int* d_idx, double* d_d2);
// correspondence set of a pair from both directions' matches: corr (na,2), *d_m = its size
PCR_HIDDEN void pcr_corr_build(pcr_ctx* ctx, const int* ij, const int* ji, int na, int mutual, int* corr, int* d_m);
// matrix-core operands of a chunk's descriptors (dup: (ng) scratch; tile_first: device [n_scans + 1]; max_norm2 zeroed by the caller)
PCR_HIDDEN void pcr_match_operands(pcr_ctx* ctx, const double* fpfh, const unsigned int* scan_first, int n_scans, size_t tiles, const unsigned int* tile_first,
                                   unsigned char* dup, double* op_t, double* op_q, double* norm2, unsigned long long* max_norm2, unsigned int* min_row);
// matching both ways, correspondence set and initial RANSAC state of every job (max_n: the largest na / nb)
PCR_HIDDEN void pcr_match_jobs(pcr_ctx* ctx, const init_job* d_jobs, int nj, int max_n, int mutual, int max_iteration);
// ---- pcr_ransac.hip
// the whole RANSAC loop over the device correspondence set (d_corr, *d_m); clouds by row.  One synchronisation.
PCR_HIDDEN int pcr_ransac_device(pcr_ctx* ctx, const pcr_pt* d_src, const pcr_pt* d_tgt, const int* d_corr, const int* d_m, const pcr_ransac_params* prm, pcr_ransac_result* res);
// iterations [c.first_iter, + c.n_iter) of the jobs d_active[0 .. n_run) (null: all of the first n_run)
PCR_HIDDEN void pcr_ransac_jobs_round(pcr_ctx* ctx, const init_job* d_jobs, const int* d_active, int n_run, const ransac_common& c);
