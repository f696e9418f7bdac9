/*
 * pcr.h -- C ABI of the MI355X-native point-cloud registration hot path.
 *
 * One shared library (libpcr.so, hipcc --offload-arch=gfx950) exports exactly
 * these symbols.  Plain C: opaque handles, caller-owned host buffers, integer
 * status codes, no exceptions across the boundary.  Every entry point names
 * the reference interface (file:line under /root/reference) it stands in for.
 *
 * Threading: a pcr_ctx owns one device and one HIP stream and is not
 * thread-safe; distinct contexts are independent.  Host arrays are only read
 * (or written) during the call.
 *
 * Arithmetic: the whole path computes in IEEE binary64 like the reference
 * (Open3D points are double; NumPy float64), with FMA contraction disabled in
 * device code so squared distances are bit-identical to
 * (dx*dx + dy*dy) + dz*dz evaluated on the host.
 */
#ifndef PCR_H
#define PCR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCR_API __attribute__((visibility("default")))

/* ---------------------------------------------------------------- status */
enum {
    PCR_OK = 0,
    /* soft status: result is valid.  Registration/main.py:125-127 prints
     * "ICP failed, cannot find enough associations!" and returns the current
     * transformation; so do we. */
    PCR_E_TOO_FEW_ASSOC = 1,
    PCR_E_INVALID = -1,     /* bad argument                                  */
    PCR_E_EMPTY = -2,       /* empty cloud (reference: IndexError/ValueError) */
    PCR_E_NOMEM = -3,
    PCR_E_HIP = -4,         /* HIP runtime error; see pcr_last_error()        */
    PCR_E_NO_DEVICE = -5,
    PCR_E_UNSUPPORTED = -6,
    PCR_E_TOO_MANY_ITERS = -7,
    PCR_E_SINGULAR = -8     /* mixture component without points or with a covariance that is not positive definite */
};

typedef struct pcr_ctx pcr_ctx;
typedef struct pcr_cloud pcr_cloud;
typedef struct pcr_index pcr_index;

PCR_API const char* pcr_strerror(int status);
PCR_API const char* pcr_last_error(const pcr_ctx* ctx); /* last HIP error text */
PCR_API const char* pcr_version(void);

/* --------------------------------------------------------------- context */
PCR_API int pcr_ctx_create(int device, pcr_ctx** out);
PCR_API int pcr_ctx_destroy(pcr_ctx* ctx);
PCR_API int pcr_ctx_sync(pcr_ctx* ctx);
/* device facts for the bench: name (<=255 chars), CU count, HBM bytes */
PCR_API int pcr_ctx_device_info(pcr_ctx* ctx, char* name256, int* cu_count, int64_t* hbm_bytes);

/* ---------------------------------------------------------------- clouds
 * Device-resident (n,3) float64 cloud stored as 32-byte records {x,y,z,id}.
 * Stands in for o3d.geometry.PointCloud.points (Registration/main.py:52-56)
 * and the (N,3) ndarrays of Kdtree_Octree/lesson2 and voxel_filter.py:19.
 * float32 input (the .bin readers, main.py:10-17) is widened exactly.       */
PCR_API int pcr_cloud_upload_f32(pcr_ctx* ctx, const float* xyz, int64_t n, int64_t stride_floats, pcr_cloud** out);
PCR_API int pcr_cloud_upload_f64(pcr_ctx* ctx, const double* xyz, int64_t n, int64_t stride_doubles, pcr_cloud** out);
PCR_API int pcr_cloud_download_f64(pcr_ctx* ctx, const pcr_cloud* cloud, double* xyz_out /* n*3 */);
PCR_API int64_t pcr_cloud_size(const pcr_cloud* cloud);
/* diagnostic: 1 when the cloud's records have been laid out along an index's curve (it was the query cloud of a grid search),
 * 0 when they are still in the caller's row order.  Results never depend on it; searches choose their path by it. */
PCR_API int pcr_cloud_reordered(const pcr_cloud* cloud);
/* diagnostic: the caller row of every record in device order (rows_out[position] = row; a permutation of [0, n), the identity
 * while pcr_cloud_reordered is 0).  A NULL pointer: PCR_E_INVALID. */
PCR_API int pcr_cloud_order(pcr_ctx* ctx, const pcr_cloud* cloud, int64_t* rows_out /* n */);
PCR_API int pcr_cloud_free(pcr_ctx* ctx, pcr_cloud* cloud);
/* Optional: lay the cloud out for queries against `index` now (its records along a Hilbert curve over the cloud's own box at the
 * index's cell, or the Morton curve with PCR_QUERY_CURVE=morton in the environment; row ids are kept, downloads are unaffected).
 * pcr_nn1 / pcr_icp do this themselves on first use. */
PCR_API int pcr_cloud_prepare(pcr_ctx* ctx, pcr_cloud* cloud, const pcr_index* index);
/* PointCloud.transform(T) in place (Registration/main.py:110), T row-major 4x4 */
PCR_API int pcr_cloud_transform(pcr_ctx* ctx, pcr_cloud* cloud, const double T[16]);

/* ----------------------------------------------------------- target index
 * Stands in for o3d.geometry.KDTreeFlann(target) (Registration/main.py:105)
 * and kdtree_construction / octree_construction
 * (Kdtree_Octree/lesson2/kdtree.py:119-137, octree.py:310-328).             */
enum { PCR_INDEX_GRID = 0, PCR_INDEX_BRUTE = 1 };
/* cell <= 0: choose the finest cell size from the cloud's extent and size */
PCR_API int pcr_index_build(pcr_ctx* ctx, const pcr_cloud* target, int kind, double cell, pcr_index** out);
PCR_API int pcr_index_free(pcr_ctx* ctx, pcr_index* index);
PCR_API int pcr_index_kind(const pcr_index* index);
PCR_API double pcr_index_cell(const pcr_index* index);
PCR_API int64_t pcr_index_size(const pcr_index* index);

/* Exact 1-NN of every query point (optionally transformed by T first) in the
 * indexed cloud: the body of the association loop Registration/main.py:116-121
 * == find_associations, icp_template.py:113-126.  idx_out[i] = target index or
 * -1 when the nearest neighbour is not closer than max_d2 (strict <, on the
 * SQUARED distance like main.py:119); max_d2 <= 0 or +inf disables the gate.
 * d2_out[i] = exact squared distance (binary64) of the reported neighbour.   */
PCR_API int pcr_nn1(pcr_ctx* ctx, const pcr_index* index, const pcr_cloud* queries, const double* T /* 16 or NULL */,
                    double max_d2, int32_t* idx_out, double* d2_out);

/* Batched k-NN / radius queries: kdtree_knn_search / octree_knn_search
 * (kdtree.py:141-172, octree.py:262-306) and *_radius_search
 * (kdtree.py:176-208, octree.py:166-259), Q queries per call.
 * knn: idx/dist are (Q,k), ascending distance, EUCLIDEAN (not squared) like
 * result_set.py; unfilled slots (k > n) hold index 0 / distance 1e10 like
 * KNNResultSet.__init__ (result_set.py:19-22).
 * radius: two-pass.  Call with idx == NULL to get counts[Q] (neighbours with
 * distance <= r, inclusive like result_set.py:80); then with offsets[Q+1]
 * (exclusive prefix sums of counts) to fill idx/dist, ascending distance.    */
PCR_API int pcr_knn(pcr_ctx* ctx, const pcr_index* index, const double* queries_xyz, int64_t q, int k,
                    int32_t* idx_out, double* dist_out);
PCR_API int pcr_radius(pcr_ctx* ctx, const pcr_index* index, const double* queries_xyz, int64_t q, double radius,
                       int64_t* counts_out, const int64_t* offsets, int32_t* idx_out, double* dist_out);

/* A handful of radius queries (q <= 64) in one call and one launch -- the reference's API is one query per call (kdtree.py:176-208,
 * octree.py:166-259): counts_out[q] = neighbours of every query; idx_out / dist_out receive the lists back to back (query i at the
 * sum of the counts before it), ascending distance, ties by index; they must hold q * cap entries.  A query with more than `cap`
 * neighbours makes the call return PCR_E_UNSUPPORTED with counts_out filled: take the two-pass pcr_radius then.                  */
PCR_API int pcr_radius_small(pcr_ctx* ctx, const pcr_index* index, const double* queries_xyz, int q, double radius, int64_t cap,
                             int64_t* counts_out, int32_t* idx_out, double* dist_out);

/* -------------------------------------------------------------------- ICP */
enum { PCR_ICP_COMPAT_MAIN = 0, /* Registration/main.py:97-156 semantics, returns LAST increment */
       PCR_ICP_TOTAL = 1        /* icp_template.py:128-200 semantics, returns composed transform */ };
enum { PCR_RMETRIC_FROBENIUS = 0, PCR_RMETRIC_GEODESIC = 1 };
#define PCR_ICP_MAX_LOG 256

typedef struct pcr_icp_params {
    int32_t max_iter;   /* main.py:98  -> 100 */
    double r_thres;     /* main.py:101 -> 0.5 */
    double t_thres;     /* main.py:102 -> 0.5 */
    double max_d2;      /* main.py:103 -> 5 (threshold on SQUARED distance) */
    int32_t mode;       /* PCR_ICP_COMPAT_MAIN | PCR_ICP_TOTAL */
    int32_t r_metric;   /* PCR_RMETRIC_* (template hint icp_template.py:184) */
    int32_t min_iter;   /* bench only: never break on the thresholds before this many solves (0 = reference behaviour);
                         * max_iter and too few associations still stop the loop */
    int32_t reserved;
} pcr_icp_params;

typedef struct pcr_icp_result {
    double T[16];          /* row-major 4x4: last increment (COMPAT) or composed (TOTAL) */
    double T_total[16];    /* composed transform in both modes                          */
    int32_t iters;         /* Procrustes solves performed                               */
    int32_t status;        /* PCR_OK or PCR_E_TOO_FEW_ASSOC                             */
    int64_t n_assoc;       /* associations of the last association pass (< 3: that pass stopped the loop) */
    double cost;           /* ||B - (R A + t)||_F of the last solve (main.py:141)       */
    double mean_d2;        /* mean squared NN distance of the last association pass     */
    double r_diff[PCR_ICP_MAX_LOG]; /* log["R_diff"], icp_template.py:189 */
    double t_diff[PCR_ICP_MAX_LOG]; /* log["t_diff"], icp_template.py:190 */
    double device_ms;      /* duration of the whole loop on the device: the kernels' own 100-MHz clock, first kernel .. the last pass's state written (device-resident loop; in a one-launch pass the wave that writes it is the last to add to the sums, not the last to leave: the kernel itself ends a microsecond or two later), HIP events otherwise */
    double nn_kernel_ms;   /* sum of HIP-event times of the pass kernels; 0 unless pcr_profile_enable(ctx, 1) (host loop: always) */
    int32_t nn_launches;   /* launches of the correspondence kernel                     */
    int32_t reserved;      /* diagnostic: 1 when the fused stages of pcr_icp_batch / pcr_register_pairs produced this result, 0 from pcr_icp (and from the batch's per-pair path) */
} pcr_icp_result;

PCR_API void pcr_icp_default_params(pcr_icp_params* p);
/* icp_point2point(source, target, transformation) (main.py:97) / ICP (icp_template.py:128).
 * `source` is updated in place exactly like main.py:110 mutates it (COMPAT) or
 * icp_template.py:195-196 (TOTAL).  max_iter <= 0: COMPAT returns T = T0, T_total = I and leaves the source alone
 * (main.py's loop body never runs); TOTAL returns T = T_total = T0 and applies T0 to the source (icp_template.py:146-152
 * applies the initial pose in front of the loop).  max_iter > PCR_ICP_MAX_LOG: PCR_E_TOO_MANY_ITERS, nothing is written. */
PCR_API int pcr_icp(pcr_ctx* ctx, pcr_cloud* source, const pcr_index* target_index, const pcr_icp_params* params,
                    const double T0[16], pcr_icp_result* result);

/* ------------------------------------------------- point-to-plane refinement
 * refine_registration (Registration/main.py:87-95): o3d registration_icp(source, target, distance_threshold,
 * result_ransac.transformation, TransformationEstimationPointToPlane()).  Open3D is absent and unpinned in the reference;
 * this follows its published algorithm ("parity unpinned"):
 *   Evaluate(T): exact nearest target q (row j) of every s = T p; a correspondence iff |s - q|^2 < max_dist^2 (strict, on
 *     the squared distance: pcr_nn1's gate); fitness = K / n_source, inlier_rmse = sqrt(sum d^2 / K), both 0 when K = 0.
 *   Update: r = (s - q) . n_j, J = [s x n_j, n_j] about the world origin, A = sum J J^T, b = sum J r, A x = -b,
 *     x = (alpha, beta, gamma, tx, ty, tz), U = [Rz(gamma) Ry(beta) Rx(alpha) | t], T <- U T.
 *   Loop: res = Evaluate(T0); for it = 1 .. max_iter: T <- Update(res) T; prev = res; res = Evaluate(T); stop when
 *     |prev.fitness - res.fitness| < rel_fitness and |prev.inlier_rmse - res.inlier_rmse| < rel_rmse.
 * Deviations: with K < 6, or A not positive definite to working precision (an LDL^T pivot d_k <= 1e-12 A_kk or not
 * finite), the update is the identity, the loop stops and the soft status is PCR_E_TOO_FEW_ASSOC (the result stays valid;
 * Open3D tests |det A| < 1e-6 instead).  The caller's source cloud is never modified (Open3D works on a copy): every pass
 * applies the composed T to the original records.                                                                        */
/* Target normals (n x 3, by target row) for the point-to-plane estimation of main.py:87-95: uploaded once, kept with the
 * index, released by pcr_index_free; a second call replaces them.  Non-finite entries -> PCR_E_INVALID; zero-length
 * normals are accepted (Open3D does not check them either).                                                               */
PCR_API int pcr_index_set_normals(pcr_ctx* ctx, pcr_index* index, const double* normals);
PCR_API int pcr_index_has_normals(const pcr_index* index); /* main.py:87-95 needs them: 1 / 0 */

typedef struct pcr_icp_plane_params {
    int32_t max_iter;     /* ICPConvergenceCriteria.max_iteration (main.py:87-95 uses Open3D's default) -> 30 */
    int32_t reserved;
    double max_dist;      /* max_correspondence_distance (main.py:89: voxel_size * 0.4); <= 0 or +inf: no gate */
    double rel_fitness;   /* -> 1e-6 */
    double rel_rmse;      /* -> 1e-6 */
} pcr_icp_plane_params;

typedef struct pcr_icp_plane_result {
    double T[16];          /* row-major 4x4: the composed transformation (RegistrationResult.transformation) */
    double fitness;        /* of the last evaluation */
    double inlier_rmse;
    int64_t n_corr;        /* correspondences of the last evaluation */
    int32_t iters;         /* updates performed */
    int32_t status;        /* PCR_OK or PCR_E_TOO_FEW_ASSOC */
    double fitness_log[PCR_ICP_MAX_LOG + 1]; /* entry 0 = evaluation of T0, entry i = evaluation after update i */
    double rmse_log[PCR_ICP_MAX_LOG + 1];
    double device_ms;      /* HIP events around the whole loop */
    int32_t nn_launches;   /* correspondence searches = evaluations */
    int32_t reserved;
} pcr_icp_plane_result;

/* Open3D's ICPConvergenceCriteria defaults as used by main.py:87-95: 30 / 1e-6 / 1e-6; max_dist = 0 (no gate) */
PCR_API void pcr_icp_plane_default_params(pcr_icp_plane_params* p);
/* registration_icp(..., TransformationEstimationPointToPlane()) of main.py:87-95 on device-resident inputs.  `index` must
 * carry normals (PCR_E_INVALID otherwise); max_iter > PCR_ICP_MAX_LOG -> PCR_E_TOO_MANY_ITERS; empty source -> PCR_E_EMPTY.
 * Returns result->status.                                                                                                */
PCR_API int pcr_icp_point2plane(pcr_ctx* ctx, const pcr_cloud* source, const pcr_index* index, const pcr_icp_plane_params* params,
                                const double T0[16], pcr_icp_plane_result* result);
/* One association + accumulation pass of main.py:87-95's estimation without a solve (counterpart of pcr_icp_moments, for
 * tests): out[0..20] = upper triangle of A row-major, out[21..26] = b, out[27] = K, out[28] = sum d^2.  T may be NULL.   */
PCR_API int pcr_point2plane_moments(pcr_ctx* ctx, const pcr_cloud* source, const pcr_index* index, const double* T, double max_dist,
                                    double out[29]);
/* The update of main.py:87-95's estimation on the host (counterpart of pcr_procrustes): solves A x = -b by LDL^T with the
 * routine the kernel runs and builds U (row-major 4x4).  PCR_E_TOO_FEW_ASSOC when A is not positive definite (x, U = identity). */
PCR_API int pcr_point2plane_solve(const double A_upper[21], const double b[6], double x[6], double U[16]);

/* Batched scan-pair registration: the loop Registration/main.py:190-216 (read pair, register, keep the pose) for many
 * independent pairs at once.  pairs[i] are caller-owned host buffers (records of `stride` values, x,y,z first: stride 6 is
 * the registration_dataset .bin record of main.py:10-17, stride 4 the KITTI record); T0 may be NULL (identity).
 * The n_ctx contexts (one device, one HIP stream each) are driven by n_ctx native worker threads that take pairs from a
 * shared counter: upload both clouds, build the grid index, run pcr_icp, free -- several pairs in flight per GPU, no
 * interpreter in the loop.  results[i] belongs to pairs[i] whatever thread ran it; status_out[i] is pcr_icp's return
 * value for that pair.  Returns the first hard error (< 0) or PCR_OK.  The contexts must not be used concurrently
 * by the caller. */
typedef struct pcr_pair {
    const float* src;     /* n_src records of stride_src floats */
    int64_t n_src;
    int64_t stride_src;
    const float* tgt;
    int64_t n_tgt;
    int64_t stride_tgt;
    const double* T0;     /* 16 doubles, row-major, or NULL */
} pcr_pair;
PCR_API int pcr_icp_batch(pcr_ctx* const* ctxs, int n_ctx, const pcr_pair* pairs, int64_t n_pairs, const pcr_icp_params* params,
                          pcr_icp_result* results, int32_t* status_out);

/* One association + accumulation pass (no solve): the 18 moments the Procrustes
 * step needs: {K, Sa[3], Sb[3], Sba[9] (row-major b_i*a_j), Saa, Sbb}, taken about
 * `origin_out[3]`.  Lets tests check the fused kernel against the oracle.      */
PCR_API int pcr_icp_moments(pcr_ctx* ctx, const pcr_cloud* source, const pcr_index* target_index, const double* T,
                            double max_d2, double moments_out[18], double origin_out[3], double* sum_d2_out);
/* procrustes_transformation(A, B) (icp_template.py:43-54, main.py:131-141) on host
 * arrays A,B laid out (3,K) row-major; R_out[9], t_out[3].                     */
PCR_API int pcr_procrustes(const double* A, const double* B, int64_t k, double R_out[9], double t_out[3], double* cost_out);
/* rotmat2quaternion / homo2tq (main.py:158-174): out = tx,ty,tz,qw,qx,qy,qz */
PCR_API int pcr_homo2tq(const double T[16], double out7[7]);

/* ----------------------------------------------------------- voxel filter
 * voxel_filter(point_cloud, leaf_size, type) (Pca_and_Voxel_filter/voxel_filter.py:10-68).
 * pcr_voxel_keys: per-point key h (float64, bit-exact, voxel_filter.py:20-33) and D[3].
 * pcr_voxel_filter: mode 0 = "centroid", 1 = "random" (explicit seed).  Output
 * rows = occupied voxels - 1 (the reference never emits its last group,
 * voxel_filter.py:42-51); out must hold n*3 doubles.
 * mode 2 = Open3D's voxel_down_sample as called at Registration/main.py:35:
 * origin min - leaf/2, every occupied voxel emitted, centroid = running sum in
 * input order / count; rows ordered by voxel key (Open3D's order is that of
 * its hash map and is not part of its contract).                             */
PCR_API int pcr_voxel_keys(pcr_ctx* ctx, const double* xyz, int64_t n, double leaf, double* h_out, double D_out[3]);
PCR_API int pcr_voxel_filter(pcr_ctx* ctx, const double* xyz, int64_t n, double leaf, int mode, uint64_t seed,
                             double* out_xyz, int64_t* n_out);
/* device-resident variant used by the downsample -> ICP pipeline (config 3) */
PCR_API int pcr_voxel_filter_cloud(pcr_ctx* ctx, const pcr_cloud* in, double leaf, int mode, uint64_t seed, pcr_cloud** out);

/* --------------------------------------------------------------------- ISS
 * Keypoint_detection_ISS/ISS.py:35-73.  lambdas_out (n,3) descending eigenvalues
 * of the weighted scatter; counts_out[n] = |N(p_i)| (self included).  "Within
 * radius" is scipy's query_ball_point, for the neighbourhoods and for the
 * suppression alike: (dx*dx + dy*dy) + dz*dz <= radius * radius in binary64
 * (not pcr_radius's sqrt(d2) <= radius, which takes up to an ulp more of d2).
 * A cloud whose largest extent exceeds 2^18 radii is refused with
 * PCR_E_UNSUPPORTED: the grid cannot hold a cell of the radius's size.
 * keypoints_out holds up to max_keypoints + 1 indices after NMS
 * (ISS.py:72-73 stops once MORE than iss_count were taken).  lambdas_out and
 * counts_out may be NULL (they are 28 bytes per point over PCIe); at least
 * one of lambdas_out / keypoints_out must be asked for.                       */
PCR_API int pcr_iss(pcr_ctx* ctx, const pcr_cloud* cloud, double radius, double gamma21, double gamma32, double nms_radius,
                    int max_keypoints, double* lambdas_out, int32_t* counts_out, int32_t* keypoints_out, int* n_keypoints_out);

/* ------------------------------------------- PCL keypoints (module PCLKeypoint)
 * The XYZ detectors of PCLKeypoints/src/keypoints.cpp: keypointHarris3D (pcl::HarrisKeypoint3D, method HARRIS) and keypointIss
 * (pcl::ISSKeypoint3D without border estimation).  PCL is not part of the build and the reference pins no version of it: the
 * rules below ARE the definition, restated in NumPy by tests/harris_checks.py; parity with PCL's binary32 output is unpinned.
 * pcr_iss above follows ISS.py and is another detector (weighted scatter, sequential suppression, a cap).
 *
 * Everything is binary64 on the stored coordinates.  N(p_i) = the rows within r of p_i, p_i included; "within r" is
 * (dx*dx + dy*dy) + dz*dz <= r*r, pcr_iss's predicate.  A cloud whose extent exceeds 2^18 radii: PCR_E_UNSUPPORTED, as pcr_iss.
 * Per-row arrays are by CALLER ROW, whatever the order of the records on the device (pcr_cloud_reordered).  Sums run in a fixed
 * order: a call is repeatable to the bit, and its results do not depend on the lay-out of the cloud's records.
 *
 * Radius normals (NormalEstimation with setRadiusSearch(r), viewpoint vp; NULL: the origin): with m = |N(p_i)| and x = p_j - p_i,
 *   cov = sum x x^T / m - mean mean^T, mean = sum x / m; the normal is the unit eigenvector of cov's smallest eigenvalue, flipped so
 *   that n . (vp - p_i) >= 0; m < 3: all three components NaN.  counts_out[i] = m.
 *
 * Harris response, from per-row normals (given, n x 3, rows without a normal hold a non-finite value; or NULL: the radius normals of
 *   the same radius): for row i with a finite normal, over the k rows of N(p_i) whose normal is finite,
 *     C = sum n_j n_j^T / k,   trace = Cxx + Cyy + Czz,
 *     det = Cxx*Cyy*Czz + 2*Cxy*Cxz*Cyz - Cxz*Cxz*Cyy - Cxy*Cxy*Czz - Cyz*Cyz*Cxx,   response = 0.04 + det - 0.04*trace*trace;
 *   the response is 0 when trace == 0, when k == 0, or when row i has no finite normal.
 *
 * Suppression (both detectors, score s): a candidate row is kept iff NO row within the suppression radius has a score strictly
 *   greater than s_i; ties keep both.  Keypoints are in ascending caller row.
 *   Harris: candidate iff response_i >= threshold; the suppression radius is `radius`.  nms == 0: every row is a keypoint.
 *
 * Refine (params.refine, only together with nms; ignored otherwise): for each kept corner position c, up to 5 rounds of
 *   A = sum n_j n_j^T, b = sum (n_j n_j^T) p_j over the rows within `radius` of c that have a finite normal; det A != 0: c <- A^-1 b
 *   (by the adjugate); a round whose squared move is <= 1e-6 is the last.  The keypoint's response stays the unrefined one.
 *
 * PCL-rule ISS: S_i = sum (p_j - p_i)(p_j - p_i)^T over N(p_i) within salient_radius, unweighted, not divided; eigenvalues
 *   e1 >= e2 >= e3; score s_i = e3 if e1 > 0, e2 > 0, e3 >= 0, e2/e1 < gamma21 and e3/e2 < gamma32, else 0.  Row i is a candidate iff
 *   s_i > 0 and |N(p_i)| within non_max_radius >= min_neighbors; suppression as above over non_max_radius.
 *   e3_out[i] = s_i (the score: 0 where a rule fails); counts_out[i] = |N(p_i)| within non_max_radius.
 *
 * Keypoints: keypoints_out holds up to `capacity` caller rows, *n_keypoints_out their number.  More keypoints than `capacity`:
 * *n_keypoints_out is the needed number, nothing is written to the per-keypoint arrays and the call returns PCR_E_UNSUPPORTED (the
 * per-row outputs are complete).  keypoint_response_out (capacity), refined_out (capacity x 3) and rounds_out (capacity; rounds of
 * the refinement, 1..5) are per keypoint and need keypoints_out.  Every output may be NULL; at least one must be asked for.          */
typedef struct pcr_harris_params {
    double radius;      /* keypoints.cpp:253  -> 0.5   */
    double threshold;   /* keypoints.cpp:254  -> 0.001 */
    int32_t nms;        /* keypoints.cpp:256  -> 0     */
    int32_t refine;     /* keypoints.cpp:257  -> 0     */
    double reserved[4];
} pcr_harris_params;
PCR_API void pcr_harris_default_params(pcr_harris_params* p);
PCR_API int pcr_normals_radius(pcr_ctx* ctx, const pcr_cloud* cloud, double radius, const double* viewpoint /* 3, or NULL */,
                               double* normals_out /* n*3 */, int32_t* counts_out /* n, or NULL */);
PCR_API int pcr_harris3d(pcr_ctx* ctx, const pcr_cloud* cloud, const double* normals /* n*3 by row, or NULL */,
                         const pcr_harris_params* params, double* response_out /* n */, int32_t* counts_out /* n: |N(p_i)| */,
                         int32_t* keypoints_out, int64_t capacity, int64_t* n_keypoints_out, double* keypoint_response_out,
                         double* refined_out, int32_t* rounds_out);
PCR_API int pcr_iss_pcl(pcr_ctx* ctx, const pcr_cloud* cloud, double salient_radius, double non_max_radius, double gamma21,
                        double gamma32, int min_neighbors, double* e3_out /* n */, int32_t* counts_out /* n */,
                        int32_t* keypoints_out, int64_t capacity, int64_t* n_keypoints_out);

/* SIFT-3D, the scale-aware detector of the module: keypointSift (keypoints.cpp:85-109, keypoints.hpp:167-178), pcl::SIFTKeypoint
 * (detectKeypoints, computeScaleSpace, findScaleSpaceExtrema) on the field the wrapper selects, the y coordinate.  As above the rules
 * below ARE the definition, restated in NumPy by tests/sift_checks.py; parity with PCL's binary32 output is unpinned.  The section's
 * conventions hold: binary64 on the stored coordinates, per-row arrays by caller row, results independent of the lay-out of the records,
 * sums in a fixed order that is a function of the cloud in caller-row order and of the radius only (a call is repeatable to the bit),
 * d2 = (dx*dx + dy*dy) + dz*dz, no operation contracted into an FMA.
 *
 * Scales of an octave, base scale b, q = n_scales_per_octave: S = q + 3 scales sigma_s = b * pow(2.0, (s - 1.0) / q), s = 0 .. S-1,
 *   computed on the host, and from them sigma2_s = sigma_s * sigma_s, lim_s = 9.0 * sigma2_s, h_s = -0.5 / sigma2_s, each rounded as
 *   written.  1 <= q <= 13 (S <= 16); any other q: PCR_E_UNSUPPORTED with a message.  pcr_sift_scales returns the sigma_s (host only).
 *
 * Response and DoG, v_j = coordinate `field` (0, 1, 2: x, y, z; the wrapper's is 1) of row j: the ball of row i is every row j with
 *   d2 <= lim_{S-1}, walked through a grid of cell 3 sigma_{S-1} (extent above 2^18 cells: PCR_E_UNSUPPORTED).  For each scale s, over the
 *   rows of the ball with d2 <= lim_s:  w = exp(d2 * h_s), num_s += v_j * w, den_s += w;  resp_s = num_s / den_s.  Row i is in every sum
 *   (w = 1), so den_s >= 1.  D[i][c] = resp_{c+1} - resp_c, c = 0 .. C-1, C = q + 2.  counts[i] = rows in the ball.
 *
 * Extrema: N(i) = the min(25, n) rows smallest in (d2, caller row), row i among them.  For c = 1 .. C-2 and val = D[i][c], the entry
 *   (i, c) is a keypoint iff fabs(val) >= min_contrast and it is
 *     a minimum: val < D[i][c-1] && val < D[i][c+1], and for no j in N(i) and no e in {c-1, c, c+1} is val > D[j][e], or
 *     a maximum: the mirrored statement.
 *   A tie with a neighbour keeps the entry, a tie with the row's own adjacent column does not.  Entries are in ascending (row, c); the
 *   keypoint's scale is sigma_c.
 *
 * Octave loop (min_scale, n_octaves, q, min_contrast): scale = min_scale, cloud = the input; for each octave cloud =
 *   voxel_down_sample(cloud, scale), stop if it holds fewer than 25 rows, run the octave above at b = scale, scale *= 2.  Keypoints are in
 *   ascending (octave, row, c) and their positions are the octave's down-sampled rows.
 *   STATED DEPARTURE: the down-sampling is mode 2 of pcr_voxel_filter_cloud (lattice origin min - leaf/2, running sum in input order, rows
 *   by voxel key).  PCL's VoxelGrid anchors its lattice at multiples of the leaf and orders its rows otherwise.
 *
 * Rows with a coordinate that is not finite: the result for such a row is unspecified (the walk stays in bounds); the Python layer
 * refuses them.  PCR_E_INVALID, before anything is launched or allocated: NULL handles, n_octaves < 1, a min_scale / base_scale that is
 * not finite and positive, a min_contrast that is NaN or negative, a field outside 0..2.  An empty cloud: PCR_E_EMPTY.
 *
 * pcr_sift_octave: one octave on the cloud as given (no down-sampling).  pcr_sift_extrema: the extrema stage alone on a caller's table
 * (n x C, host, 3 <= C <= 15).  pcr_sift: the loop; the octaves' clouds stay on the device.  keypoints_out: x, y, z, scale per keypoint;
 * octave_out / row_out (or NULL): its octave and its row of that octave's cloud; octave_sizes_out (n_octaves, or NULL): the rows of each
 * octave's cloud, 0 for the octaves not run.  The capacity rule is pcr_harris3d's: on more entries than `capacity`, *n_out is the needed
 * number, nothing is written to the per-keypoint arrays and the call returns PCR_E_UNSUPPORTED (the per-row outputs are complete).        */
PCR_API int pcr_sift_scales(double base_scale, int n_scales_per_octave, double* scales_out /* n_scales_per_octave + 3 */);
PCR_API int pcr_sift_octave(pcr_ctx* ctx, const pcr_cloud* cloud, double base_scale, int n_scales_per_octave, double min_contrast, int field,
                            double* dog_out /* n*C, or NULL */, int32_t* counts_out /* n, or NULL */, int32_t* rows_out, int32_t* cols_out,
                            int64_t capacity, int64_t* n_out);
PCR_API int pcr_sift_extrema(pcr_ctx* ctx, const pcr_cloud* cloud, const double* dog /* n*C by row, host */, int n_columns, double min_contrast,
                             int32_t* rows_out, int32_t* cols_out, int64_t capacity, int64_t* n_out);
PCR_API int pcr_sift(pcr_ctx* ctx, const pcr_cloud* cloud, double min_scale, int n_octaves, int n_scales_per_octave, double min_contrast, int field,
                     double* keypoints_out /* capacity*4 */, int32_t* octave_out, int32_t* row_out, int64_t capacity, int64_t* n_out,
                     int64_t* octave_sizes_out);

/* PCL-rule descriptors of the same module: featureFPFH33(pointcloud, keypoints, compute_normal_k, feature_radius) and
 * featureFPFH33WithNormal(pointcloud, normals, keypoints, feature_radius) (keypoints.cpp:112-184,272-281) are pcr_normals_knn followed
 * by pcr_fpfh_pcl, or pcr_fpfh_pcl alone.  As for the keypoints, the rules below ARE the definition (restated in NumPy by
 * tests/pcl_fpfh_checks.py); parity with PCL's binary32 output is unpinned.  The conventions of the section hold: binary64 on the
 * stored coordinates, per-row arrays by caller row, results independent of the lay-out of the records, PCR_E_UNSUPPORTED for a cloud
 * whose extent exceeds 2^18 radii.  pcr_fpfh / pcr_fpfh_rows follow Open3D's rules (hybrid neighbourhood, max_nn cap, the row's own
 * SPFH added on top) and are other descriptors.
 *
 * Ball: B(x) = the surface rows j with (dx*dx + dy*dy) + dz*dz <= r*r, d = p_j - x: the predicate above.  No cap: a ball may hold
 *   every row of the cloud.
 *
 * k-NN normals (pcr_normals_knn: NormalEstimation with setKSearch(k), viewpoint vp; NULL: the origin): the neighbourhood of row i is its
 *   k nearest rows, itself included, ordered by (distance, row) -- pcr_normals' neighbourhood, and its covariance; the normal is the
 *   unit eigenvector of the covariance's smallest eigenvalue, flipped so that n . (vp - p_i) >= 0; curvature = e_min / (e0 + e1 + e2),
 *   and 0 when that sum is 0.  A neighbourhood of fewer than 3 rows (a cloud of n < 3 rows): NaN, normal and curvature.  Supported:
 *   3 <= k <= 16, what the exact batched k-NN supports; any other k: PCR_E_UNSUPPORTED with a message (pcr_last_error).
 *
 * SPFH of surface row i, from per-row normals (n x 3 by caller row; rows without one hold a non-finite value): K = |B(p_i)|.  Every
 *   j in B(p_i) with j != i (by row number) forms a pair (p_i, n_i, p_j, n_j) with the Darboux-frame features of pcr_fpfh's SPFH --
 *   d = p_j - p_i, a1 = n_i.d/|d|, a2 = n_j.d/|d|; if |a1| < |a2| the pair is swapped (u = n_j, w = n_i, d = -d, f2 = -a2), else
 *   u = n_i, w = n_j, f2 = a1; v = (d x u)/|d x u|; f1 = v.w; f0 = atan2((u x v).w, u.w), written in that order.  The pair is SKIPPED
 *   -- not binned -- when |d| == 0, when |d x u| == 0, or when a component of n_i or n_j is not finite.  Otherwise it adds 1 to the bins
 *     clamp(floor(11 (f0 + pi) / (2 pi))),  11 + clamp(floor(11 (f1 + 1) 0.5)),  22 + clamp(floor(11 (f2 + 1) 0.5)),  clamp to 0..10.
 *   With c_b the integer count of bin b: spfh_i[b] = c_b * (100.0 / (K - 1)) -- one product, one rounding -- and 0 when K == 1.
 *   K counts every row of the ball, skipped pairs included.
 *
 * FPFH33 at keypoint x (any coordinates, on the surface or not): F[b] = sum over j in B(x) with d2_j != 0 of spfh_j[b] / d2_j (a true
 *   division, d2_j = the predicate's left side); per block of 11 bins, with s the sum of the block's F in bin order,
 *   out[b] = F[b] * (s != 0 ? 100.0 / s : 0.0).  The keypoint's own SPFH is NOT added.  An empty B(x), or an x with a component that is
 *   not finite: 33 NaN (counts_out 0).  A ball that holds only rows at distance 0: 33 zeros.  A keypoint outside the cloud's box meets
 *   empty space like any other.  The sum over j runs in a fixed order that is a function of the surface in caller-row order and of
 *   the radius only (the grid cells of size r in a fixed order around x's cell, caller-row order within a cell): not of m, not of
 *   the other keypoints, not of the lay-out of the records.  A call is repeatable to the bit.
 *
 * pcr_fpfh_pcl: surface = the cloud; normals (n,3) by caller row and keypoints (m,3), both on the host; features_out (m,33) row-major
 *   binary64 (PCL's float is this rounded once); counts_out (m, may be NULL) = |B(x)|; *n_spfh_out (may be NULL) = M, the rows whose
 *   SPFH was computed: the size of the union of the keypoints' balls.  NULL handles or arrays, m < 0, or a radius that is not a finite
 *   positive number: PCR_E_INVALID before anything is launched or allocated.  m == 0: PCR_OK, nothing written, *n_spfh_out = 0.       */
PCR_API int pcr_normals_knn(pcr_ctx* ctx, const pcr_cloud* cloud, int k, const double* viewpoint /* 3, or NULL */, double* normals_out /* n*3 */,
                            double* curvature_out /* n, or NULL */);
PCR_API int pcr_fpfh_pcl(pcr_ctx* ctx, const pcr_cloud* surface, const double* normals /* (n,3) by caller row, host */,
                         const double* keypoints /* (m,3), host */, int64_t m, double radius, double* features_out /* (m,33) binary64 */,
                         int32_t* counts_out /* m, or NULL: |B(x)| */, int64_t* n_spfh_out /* or NULL: M */);

/* SHOT352 at keypoint positions: featureSHOT352(pointcloud, keypoints, compute_normal_k, feature_radius) and
 * featureSHOT352WithNormal(pointcloud, normals, keypoints, feature_radius) (keypoints.cpp:187-235,282-291) are pcr_normals_knn followed
 * by pcr_shot352, or pcr_shot352 alone.  The rules below ARE the definition (restated in NumPy by tests/shot_checks.py):
 * parity with PCL's binary32 output is unpinned.  The conventions of the section hold: binary64 on the stored coordinates, per-row
 * arrays by caller row, results independent of the lay-out of the records, PCR_E_UNSUPPORTED for a cloud whose extent exceeds 2^18
 * radii, the ball B(x) of pcr_fpfh_pcl with no cap.  Every dot product is taken in the written order (a0*b0 + a1*b1) + a2*b2 and nothing is
 * contracted into a fused multiply-add: the hard decisions below are then the same bits wherever they are evaluated.
 *
 * Local reference frame at keypoint x (any finite coordinates, on the surface or not; SHOTLocalReferenceFrameEstimation): K = |B(x)|;
 *   for j in B(x): v_j = p_j - x, d2_j = (v0*v0 + v1*v1) + v2*v2, d_j = sqrt(d2_j), w_j = r - d_j.  M = (sum w_j v_j v_j^T) / (sum w_j):
 *   six moments ((w_j v_a) v_b each) and the weight sum, each moment divided by the weight sum.  K < 5, or a weight sum that is not
 *   positive (every row at distance r): the frame is 9 NaN and the descriptor 352 NaN.  Eigenvalues e0 <= e1 <= e2 of M; the x axis
 *   is the unit eigenvector of e2, the z axis that of e0, each first given the sign that makes its component of largest magnitude
 *   positive (the first such of equal magnitudes): rows AT the keypoint count as plus for a and for -a, so both can satisfy the rule
 *   that follows, and the frame must not depend on the eigen solver.  Sign of an axis a: P = #{j in B(x) : v_j.a >= 0} (the zero vector counts as
 *   plus), s = 2P - K; s < 0: a is negated; s > 0: it stays; s == 0: of the five neighbours of ranks K/2-2 .. K/2+2 (integer division)
 *   in ascending (d2_j, caller row) order, those with v_j.a > 0 (strictly) are counted, and a is negated when they are fewer than 3.
 *   x and z are decided independently; y = z cross x, taken after both signs.  The frame is stored as rows x, y, z: (m,9) row-major.
 *   The moment sums run in a fixed order that is a function of the surface in caller-row order, of the radius and of x's grid cell
 *   only (pcr_fpfh_pcl's contract): a call is repeatable to the bit and a keypoint does not depend on the others.
 *
 * Histogram, 352 = 32 volumes x 11 slots, from a frame (rows X, Y, Z axes) with nine finite entries; any other frame: 352 NaN.
 *   Constants: r4 = 0.25 r, r2 = 0.5 r, r34 = 0.75 r; q4, q2, q34, q78 = the doubles nearest pi/4, pi/2, 3 pi/4, 7 pi/8.
 *   A neighbour j in B(x) is SKIPPED when a component of its normal n_j is not finite or when d2_j == 0.  Otherwise
 *     c = clamp(n_j.Z, -1, 1);  b = ((1.0 + c) * 10) / 2;  X = v_j.Xaxis, Y = v_j.Yaxis, Z = v_j.Zaxis, each set to 0 when its
 *     magnitude is < 1e-30;  d = sqrt(d2_j).
 *   Volume: bit4 = (Y > 0) || (Y == 0 && X < 0);  bit3 = ((X > 0) || (X == 0 && Y > 0)) ? !bit4 : bit4;
 *     desc = ((bit4 << 3) + (bit3 << 2)) << 1;  if (X*Y > 0 || X == 0) desc += (|X| >= |Y|) ? 0 : 4; else desc += (|X| > |Y|) ? 4 : 0;
 *     desc += (Z > 0) ? 1 : 0;  desc += (d > r2) ? 2 : 0;  sel = desc >> 2 (the azimuth sector, centre -q78 + q4*sel).
 *   Cosine: step = floor(b + 0.5) (0..10), rho = b - step, vol = 11 desc, W = 1 - |rho|;
 *     rho > 0: h[vol + (step + 1) % 10] += rho;  else: h[vol + (step - 1 + 10) % 10] += -rho.
 *   Radial: d > r2: t = (d - r34) / r2;  d > r34: W += 1 - t;  else W += 1 + t and h[11 (desc - 2) + step] += -t.
 *           else:   t = (d - r4) / r2;   d < r4:  W += 1 + t;  else W += 1 - t and h[11 (desc + 2) + step] += t.
 *   Elevation: theta = acos(clamp(Z / d, -1, 1)).
 *           Z <= 0: u = (theta - q34) / q2;  theta > q34: W += 1 - u;  else W += 1 + u and h[11 (desc + 1) + step] += -u.
 *           else:   u = (theta - q4) / q2;   theta < q4:  W += 1 + u;  else W += 1 - u and h[11 (desc - 1) + step] += u.
 *   Azimuth, only when X != 0 or Y != 0: a = clamp((atan2(Y, X) - (-q78 + q4 * sel)) / q4, -0.5, 0.5);
 *           a > 0: W += 1 - a and h[11 ((desc + 4) % 32) + step] += a;  else W += 1 + a and h[11 ((desc - 4 + 32) % 32) + step] += -a.
 *   Last: h[vol + step] += W.
 *   Accumulation: every added value v enters as the integer rint(v * 2^32) (ties to even; W once, after its binary64 sum in the order
 *   above), the integers are summed as 64-bit integers -- exact in any order, no overflow below 2^28 rows in a ball -- and
 *   h_b = (double)integer * 2^-32.  Output: out_b = h_b / sqrt(sum h_b^2), the sum in bin order to within rounding.  A zero norm (every
 *   neighbour skipped) gives 352 NaN: PCL's 0/0.  An x that is not finite: count 0, NaN frame, NaN descriptor.
 *
 * pcr_shot_lrf: frames_out (m,9); counts_out (m, may be NULL) = |B(x)|.
 * pcr_shot352: normals (n,3) by caller row and keypoints (m,3), on the host; features_out (m,352) row-major binary64 (PCL's float is
 *   this rounded once).  frames_in NULL: the frames above are computed.  frames_in (m,9): it replaces the frame stage
 *   (setInputReferenceFrames) -- whatever K is; a row with an entry that is not finite gives 352 NaN.  frames_out (may be NULL) echoes
 *   the frames used: features_out with frames_in = an earlier call's frames_out has that call's bytes.  NULL handles or arrays, m < 0,
 *   m > 2^31 - 1, or a radius that is not a finite positive number: PCR_E_INVALID before anything is launched or allocated.  m == 0:
 *   PCR_OK, nothing written.  An empty surface: PCR_E_EMPTY.                                                                         */
PCR_API int pcr_shot_lrf(pcr_ctx* ctx, const pcr_cloud* surface, const double* keypoints /* (m,3), host */, int64_t m, double radius,
                         double* frames_out /* (m,9) */, int32_t* counts_out /* m, or NULL */);
PCR_API int pcr_shot352(pcr_ctx* ctx, const pcr_cloud* surface, const double* normals /* (n,3) by caller row, host */,
                        const double* keypoints /* (m,3), host */, int64_t m, double radius, const double* frames_in /* (m,9), or NULL: computed */,
                        double* features_out /* (m,352) binary64 */, double* frames_out /* (m,9), or NULL */, int32_t* counts_out /* m, or NULL */);

/* ---------------------------------------------------------- PCA / normals
 * pcr_pca: Pca_and_Voxel_filter/pca_normal.py:10-36 PCA(data, sort=True):
 * eigen-decomposition of np.cov of the cloud (divisor n-1); eigvals_out
 * descending, eigvecs_out row-major 3x3 whose COLUMNS are the eigenvectors
 * (sign arbitrary, like LAPACK's in the reference).  mean_out may be NULL.
 * pcr_normals: pca_normal.py:85-90 -- for every point the eigenvector of the
 * smallest eigenvalue of the covariance of its k nearest neighbours (the point
 * itself included, like search_knn_vector_3d on a cloud point); 2 <= k <= 16.
 * normals_out (n,3) by caller row; eigvals_out (n,3) descending and
 * neighbours_out (n,k) ascending (distance, index) may be NULL.  A cloud of
 * n < k points: every row holds the n points in that order, then -1, and the
 * covariance is of the n points (divisor n-1).  n = 1: the covariance is taken
 * as zero -- eigenvalues 0, normal (0,0,1), neighbours 0 then -1.            */
PCR_API int pcr_pca(pcr_ctx* ctx, const pcr_cloud* cloud, double eigvals_out[3], double eigvecs_out[9], double mean_out[3]);
PCR_API int pcr_normals(pcr_ctx* ctx, const pcr_cloud* cloud, int k, double* normals_out, double* eigvals_out,
                        int32_t* neighbours_out);

/* ------------------------------------------- global initialisation (next row)
 * The Open3D stage in front of ICP, Registration/main.py:33-84, and the template
 * surface icp_template.py:20-41,56-110.  Open3D is absent and unpinned in the
 * reference; these follow its published behaviour ("parity unpinned").
 * pcr_normals_hybrid: estimate_normals(KDTreeSearchParamHybrid(radius, max_nn))
 *   (main.py:39-40): neighbourhood = the <= max_nn nearest points with
 *   d^2 < radius^2; fewer than 3 -> (0,0,1).  orient != 0 flips every normal
 *   toward viewpoint[3] (NULL = origin); orient == 0 leaves the solver's sign.
 * pcr_fpfh: compute_fpfh_feature (main.py:44-46); normals (n,3) by row;
 *   features_out (n,33) row-major (= Open3D's Feature.data (33,n) column-major).
 * pcr_fpfh_rows: the descriptors of m chosen rows (keypoints described over the
 *   cloud as search surface).  features_out[i] (m,33) holds, bit for bit, row
 *   rows[i] of what pcr_fpfh writes for the same cloud, normals, radius and
 *   max_nn; rows may be in any order and may repeat.  Only the SPFH of the rows
 *   that the chosen rows' neighbour lists reach is computed: *n_spfh_out (may be
 *   NULL) receives how many distinct rows that were -- the size of the union of
 *   the lists, each of which holds its own row (a row with max_nn or more exact
 *   duplicates of lower row number in front of it is counted besides its list).
 *   NULL arguments, m < 0 or a row outside [0, n): PCR_E_INVALID before anything
 *   is launched or allocated; m == 0: PCR_OK, nothing written, *n_spfh_out = 0;
 *   every other status as pcr_fpfh reports it.
 * pcr_feature_match: nearest target row in feature space for every query row
 *   (find_matchings, icp_template.py:20-41); squared L2, ties to the lowest row.
 * pcr_ransac: registration_ransac_based_on_feature_matching's loop
 *   (main.py:73-83) / ransac_init's loop (icp_template.py:88-110) over a given
 *   correspondence set corr (m,2) of (source row, target row): 3 samples,
 *   edge-length and distance checkers, Kabsch, inliers counted over corr,
 *   running best in iteration order with the confidence-based early exit.    */
typedef struct pcr_ransac_params {
    int32_t max_iteration;
    int32_t check_distance;
    double confidence;
    double max_distance;
    double edge_similarity; /* <= 0 switches the edge-length checker off */
    uint64_t seed;
    double reserved[4];
} pcr_ransac_params;
typedef struct pcr_ransac_result {
    double T[16];
    int32_t iterations, n_valid, best_iteration, reserved_i;
    double corr_fitness, corr_rmse;
    double reserved[4];
} pcr_ransac_result;
PCR_API int pcr_normals_hybrid(pcr_ctx* ctx, const pcr_cloud* cloud, double radius, int max_nn, int orient, const double viewpoint[3],
                               double* normals_out);
PCR_API int pcr_fpfh(pcr_ctx* ctx, const pcr_cloud* cloud, const double* normals, double radius, int max_nn, double* features_out);
PCR_API int pcr_fpfh_rows(pcr_ctx* ctx, const pcr_cloud* cloud, const double* normals /* (n,3) by caller row, host */, double radius, int max_nn,
                          const int64_t* rows /* m caller rows, host */, int64_t m, double* features_out /* (m,33) row-major, host */,
                          int64_t* n_spfh_out /* may be NULL */);
PCR_API int pcr_feature_match(pcr_ctx* ctx, const double* queries, int64_t nq, const double* targets, int64_t nt, int dim,
                              int32_t* idx_out, double* d2_out);
PCR_API int pcr_ransac_default_params(pcr_ransac_params* p);
PCR_API int pcr_ransac(pcr_ctx* ctx, const pcr_cloud* source, const pcr_cloud* target, const int32_t* corr, int64_t m,
                       const pcr_ransac_params* params, pcr_ransac_result* result);

/* Device-resident variant of the same stage -- what the pair loop main.py:190-216 runs per pair, without a host round trip
 * between its steps.
 * pcr_preprocess = preprocess_point_cloud(pcd, voxel_size) (main.py:33-47): voxel_down_sample(voxel_size) (mode 2 of
 *   pcr_voxel_filter), estimate_normals(Hybrid(normal_radius, normal_max_nn)) oriented toward the origin,
 *   compute_fpfh_feature(Hybrid(fpfh_radius, fpfh_max_nn)); main.py:39,44 use 2 x / 5 x voxel_size and 30 / 100.  The result
 *   (down-sampled cloud, normals, 33-d descriptors) stays on the device in a pcr_prep, to be used for every pair the scan
 *   takes part in (342 pairs over 504 scans in Registration/reg_result.txt).  A pcr_prep belongs to the context that made it
 *   (pcr_prep_free with that context) but may be READ by any context of the same device once pcr_preprocess has returned.
 * pcr_global_registration = execute_global_registration (main.py:68-84): nearest descriptors both ways, mutual filter (falls
 *   back to the one-way set below 9 survivors, like Open3D), pcr_ransac's loop over that set; result->reserved_i = size of
 *   the correspondence set.  The final whole-cloud evaluation Open3D appends (fitness / inlier_rmse of the RegistrationResult)
 *   is not part of it: main.py:211 reads .transformation only.                                                            */
typedef struct pcr_prep pcr_prep;
PCR_API int pcr_preprocess(pcr_ctx* ctx, const pcr_cloud* cloud, double voxel_size, double normal_radius, int normal_max_nn,
                           double fpfh_radius, int fpfh_max_nn, pcr_prep** out);
PCR_API int64_t pcr_prep_size(const pcr_prep* prep);
PCR_API const pcr_cloud* pcr_prep_cloud(const pcr_prep* prep);   /* the down-sampled cloud (owned by the prep) */
/* points (n,3), normals (n,3), features (n,33) row-major; any of them may be NULL */
PCR_API int pcr_prep_download(pcr_ctx* ctx, const pcr_prep* prep, double* points, double* normals, double* features);
PCR_API int pcr_prep_free(pcr_ctx* ctx, pcr_prep* prep);
PCR_API int pcr_global_registration(pcr_ctx* ctx, const pcr_prep* source, const pcr_prep* target, const pcr_ransac_params* params,
                                    int mutual_filter, pcr_ransac_result* result);

/* The whole pair loop of Registration/main.py:183-216 over a table of scans: pairs[i] = (source scan, target scan) as indices
 * into clouds[] (the rows "trg,src" of the pair list, main.py:186-194; clouds[] = the <id>.bin files read by read_bin_velodyne,
 * main.py:10-17).  A scan that takes part in several pairs (Registration/reg_result.txt: 342 pairs over 504 scans) is uploaded
 * and, with `global`, preprocessed ONCE per call and kept on the device while the call runs.
 *   global != NULL: prepare_dataset + execute_global_registration (main.py:196-203) give the initial transform of every pair
 *     whose T0 is NULL: pcr_preprocess of every scan such a pair uses, pcr_global_registration per pair (the same ransac seed
 *     for every pair, so a pair's result does not depend on which other pairs share the call); a pair for which no hypothesis
 *     passes the checkers starts from identity.  T_init_out (n_pairs x 16, may be NULL) receives the transforms ICP started from.
 *     (Inside, the stage runs fused for the whole call on the first context -- every scan down-sampled by one sort, every later step
 *     one launch for all scans / all pairs -- and scan by scan for a share that does not fit that path: the same results bit for bit.)
 *   then icp_point2point (main.py:211) for every pair through pcr_icp_batch's fused stages.
 * results / status_out as pcr_icp_batch.                                                                                   */
typedef struct pcr_cloud_ref {
    const float* xyz;     /* n records of `stride` floats, x, y, z first */
    int64_t n;
    int64_t stride;
} pcr_cloud_ref;
typedef struct pcr_pair_ref {
    int32_t src, tgt;     /* rows of clouds[] */
    const double* T0;     /* 16 doubles, row-major, or NULL (identity, or the global registration's result) */
} pcr_pair_ref;
typedef struct pcr_global_params {
    double voxel_size;        /* main.py:196 -> 2.0 */
    double normal_radius;     /* main.py:38  -> voxel_size * 2 */
    double fpfh_radius;       /* main.py:43  -> voxel_size * 5 */
    int32_t normal_max_nn;    /* main.py:40  -> 30 */
    int32_t fpfh_max_nn;      /* main.py:46  -> 100 */
    int32_t mutual_filter;    /* main.py:74  -> 1 */
    int32_t reserved_i;
    pcr_ransac_params ransac; /* main.py:70-83 -> max_distance voxel_size * 1.5, edge 0.9, 100000 iterations / 0.999 */
} pcr_global_params;
PCR_API int pcr_global_default_params(double voxel_size, pcr_global_params* p);
PCR_API int pcr_register_pairs(pcr_ctx* const* ctxs, int n_ctx, const pcr_cloud_ref* clouds, int64_t n_clouds, const pcr_pair_ref* pairs,
                               int64_t n_pairs, const pcr_global_params* global, const pcr_icp_params* icp, pcr_icp_result* results,
                               int32_t* status_out, double* T_init_out);
/* DIAGNOSTIC entry point -- a seam for tests, not part of the pair loop: the fused initialisation's matching step alone, on
 * descriptors the caller brings.  descriptors (ng,33) row-major hold n_sets descriptor sets one behind the other, set s = rows
 * [set_first[s], set_first[s + 1]) (set_first[0] = 0, every set non-empty); pair_sets (n_pairs,2) = (source set, target set).
 * The sets are turned into the matrix-core operands and matched exactly as the scans of a share are (one launch for all pairs;
 * how the targets are split depends on the number of pairs and the device).  Outputs, pair behind pair in the order given:
 * ij_out / dab_out (na per pair): nearest target row of every source row and its squared distance; ji_out / dba_out (nb per
 * pair): the other way (written only with mutual_filter); corr_out (na,2 per pair) of which the first m_out[pair] rows are the
 * correspondence set pcr_global_registration would sample from.  A set above 4096 rows: PCR_E_UNSUPPORTED (the fused path
 * declines such scans); more than 2048 sets, an empty set, a set index out of range: PCR_E_INVALID.                      */
PCR_API int pcr_match_pairs_fused(pcr_ctx* ctx, const double* descriptors, const int64_t* set_first, int64_t n_sets, const int32_t* pair_sets,
                                  int64_t n_pairs, int mutual_filter, int32_t* ij_out, double* dab_out, int32_t* ji_out, double* dba_out,
                                  int32_t* corr_out, int32_t* m_out);

/* ------------------------------------------------------------------ DBSCAN
 * DBSCAN.fit (Cluster_dbscan/dbscan.py:10-36):
 * labels_out[n] = cluster id per row (-1 noise), numbered in the reference's
 * discovery order (seeds taken from the END of the index list; a seed needs
 * >= min_pts neighbours, a reached point expands only with > min_pts; a point
 * first met as a noise seed stays noise).  Neighbourhood = the point itself and
 * every point with (dx*dx + dy*dy) + dz*dz <= radius * radius in binary64 (scipy
 * query_ball_point; not pcr_radius's sqrt(d2) <= radius, see pcr_iss).        */
PCR_API int pcr_dbscan(pcr_ctx* ctx, const pcr_cloud* cloud, double radius, int min_pts, int32_t* labels_out, int32_t* n_clusters_out);

/* ------------------------------------------------------ ground segmentation
 * ground_segmentation (Cluster_dbscan/clustering.py:36-95), the step in front of DBSCAN in its main() (clustering.py:158-160):
 * RANSAC plane fit, the inliers of the best plane removed.  Trial j takes the rows samples[3j .. 3j+2] (the caller draws them:
 * clustering.py:57 uses np.random, and the library has no generator for this step), p0,p1,p2 = their points,
 *   c = cross(p0 - p1, p0 - p2), nrm = c / sqrt((cx*cx + cy*cy) + cz*cz)       (a degenerate triple: 0/0 = NaN, like the reference)
 *   row i is an inlier iff |((vx*nx + vy*ny) + vz*nz)| < tau, v = point_i - p0   (strict; false for NaN)
 * in binary64 on the stored coordinates, this operation order, no contraction: a NumPy float64 restatement agrees on every point.
 * (The reference evaluates in float32 because its reader returns float32: labels can differ only within a rounding band of tau.)
 * The running best is replaced on a strictly larger count (the earlier of two equal trials wins), and right after a replacement
 * the loop breaks when best / n > ratio (clustering.py:75-81).  Every hypothesis is scored whatever the break: counts_out holds
 * all n_hyp true counts, `evaluated` says how many trials the reference would have run.
 * Outputs, each optional: the outlier rows of the winner in ascending row order as a new device-resident cloud (ids 0..m-1, no
 * bounding box, not reordered; m may be 0) and as a row list (first n_outliers entries), the inlier flag of every row.
 * Every trial degenerate (clustering.py:83 indexes with None): PCR_E_TOO_FEW_ASSOC, no cloud, best_hyp = -1, counts_out valid.
 * PCR_E_INVALID: tau not finite, n_hyp < 1, a sample row outside [0, n), NULL samples / params / result.  Empty cloud: PCR_E_EMPTY. */
typedef struct pcr_ground_params {
    double tau;           /* clustering.py:17 -> 0.6 */
    double ratio;         /* clustering.py:19 -> 0.5 */
    int32_t n_hyp;        /* clustering.py:18 -> 35  */
    int32_t reserved_i;
    double reserved[4];
} pcr_ground_params;
typedef struct pcr_ground_result {
    int32_t best_hyp, evaluated;  /* winning trial; trials the reference would have run (break trial + 1, or n_hyp) */
    int64_t n_inliers, n_outliers;
    double point[3], normal[3];   /* p0 and unit normal of the winner */
    double reserved[4];
} pcr_ground_result;
PCR_API void pcr_ground_default_params(pcr_ground_params* p);   /* 0.6, 0.5, 35 */
/* The running-best / early-break rule of clustering.py:75-81 over the counts of all trials, on the host -- the source the device's
 * finishing step compiles (counterpart of pcr_point2plane_solve).  The break test is (double)best / (double)n > ratio.
 * PCR_E_TOO_FEW_ASSOC when no count is positive (best_hyp = -1, evaluated = n_hyp); PCR_E_INVALID: NULL pointer, n_hyp < 1,
 * n < 1, a count outside [0, n].                                                                                              */
PCR_API int pcr_ground_select(const int64_t* counts, int32_t n_hyp, int64_t n, double ratio, int32_t* best_hyp, int32_t* evaluated);
PCR_API int pcr_ground_segmentation(pcr_ctx* ctx, const pcr_cloud* cloud, const int64_t* samples /* n_hyp x 3 caller rows */,
                                    const pcr_ground_params* params, pcr_cloud** outliers_out /* NULL = not wanted */,
                                    int32_t* outlier_rows_out /* n or NULL */, uint8_t* inlier_mask_out /* n or NULL */,
                                    int64_t* counts_out /* n_hyp or NULL: every hypothesis's true count */, pcr_ground_result* result);

/* ------------------------------------------------------------- Gaussian mixture
 * class GMM (Cluster_KMeans_GMM/GMM.py:13-71): EM with full covariances on a device-resident cloud.
 *   init (GMM.py:25-27): the caller's means0 (the reference draws np.random.random((k, dim))), covariances I, weights 1/k, last_nll = inf
 *   E (GMM.py:31-35):  gamma[k,n] ~ w_k N(x_n; mu_k, Sigma_k), normalised over k
 *   M (GMM.py:38-53):  N_k = sum gamma; mu_k = sum gamma x / N_k; Sigma_k = sum gamma (x - mu_k)(x - mu_k)^T / N_k about the NEW means
 *                      with the SAME gamma, no regularisation; w_k = N_k / n
 *   stop (GMM.py:56-63): nll = -sum_n log sum_k w_k N(x_n; .) of the NEW parameters; last_nll - nll < tol: break (the updated
 *                      parameters stay); else last_nll = nll
 *   predict (GMM.py:65-70): argmax_k w_k N(x; mu_k, Sigma_k), the lowest k on ties.
 * Deviation 1, the log domain: Sigma_k = L L^T, a_k(x) = log w_k - dim/2 log 2pi - sum_i log L_ii - |L^-1 (x - mu_k)|^2 / 2,
 *   m = max_k a_k, gamma_k = exp(a_k - m) / sum_j exp(a_j - m), log-likelihood of the point = m + log sum_j exp(a_j - m).  Equal to
 *   the reference to rounding wherever its densities do not underflow, and defined where it gives 0/0 (any point more than ~38
 *   units from every mean of an identity-covariance start).
 * Deviation 2, failure: a component whose N_k is 0 or not finite, or whose covariance has a Cholesky pivot that is not positive or
 *   not finite, ends pcr_gmm_fit with PCR_E_SINGULAR; result->bad_iter / bad_component name the iteration (1-based) and the
 *   component (scipy raises LinAlgError / ValueError at that point); the outputs are not written.
 * Limits: 1 <= k <= PCR_GMM_MAX_K, dim 2 or 3 (dim 2 uses x and y of the records and ignores z), max_iter >= 1: otherwise
 *   PCR_E_INVALID; an empty cloud: PCR_E_EMPTY.  means (k,dim), covs (k,dim,dim), weights (k) row-major; of a covariance the lower
 *   triangle is read.  Sums are taken in a fixed order without floating-point atomics: two calls give the same bits.           */
#define PCR_GMM_MAX_K 32
typedef struct pcr_gmm_params {
    int32_t n_clusters;   /* GMM.py:14 */
    int32_t dim;          /* data.shape[1]: 2 or 3 -> 3 */
    int32_t max_iter;     /* GMM.py:14 -> 50 */
    int32_t reserved_i;
    double tol;           /* GMM.py:14 -> 0.001 */
    double reserved[4];
} pcr_gmm_params;
typedef struct pcr_gmm_result {
    int32_t iters;          /* EM iterations performed (trips of the loop GMM.py:29) */
    int32_t converged;      /* the loop broke on the rule of GMM.py:61 */
    int32_t bad_component;  /* PCR_E_SINGULAR: the (lowest) failing component, -1 otherwise */
    int32_t bad_iter;       /* PCR_E_SINGULAR: the iteration it failed in, 1-based */
    double nll;             /* negative log-likelihood of the returned parameters */
    double device_ms;       /* HIP events around the whole loop */
    int32_t passes;         /* streaming passes over the cloud the loop needs: 2 iters + 1 */
    int32_t reserved_i;
    double reserved[4];
} pcr_gmm_result;
PCR_API void pcr_gmm_default_params(pcr_gmm_params* p);   /* 1 cluster, dim 3, 50, 0.001 */
/* GMM.fit (GMM.py:23-63), the whole loop with its state on the device.  nll_hist_out (max_iter entries or NULL): nll after every
 * iteration, the first result->iters entries are written.                                                                     */
PCR_API int pcr_gmm_fit(pcr_ctx* ctx, const pcr_cloud* cloud, const pcr_gmm_params* params, const double* means0 /* k*dim */, double* means_out,
                        double* covs_out /* k*dim*dim */, double* weights_out /* k */, double* nll_hist_out, pcr_gmm_result* result);
/* Exactly one E + M step (GMM.py:31-53) from the given parameters, for callers with their own loop and for tests: the new
 * parameters, N_k, and *loglik_in_out = the log-likelihood of the INPUT parameters.  The status comes from the input parameters
 * only (PCR_E_SINGULAR: an input covariance is not positive definite); what an empty component gives (0/0) is returned as it is.
 * Every output may be NULL.                                                                                                   */
PCR_API int pcr_gmm_step(pcr_ctx* ctx, const pcr_cloud* cloud, int k, int dim, const double* means, const double* covs, const double* weights,
                         double* means_out, double* covs_out, double* weights_out, double* nk_out, double* loglik_in_out);
/* GMM.predict (GMM.py:65-70): labels_out[n] by caller row; resp_out (n,k) or NULL: the responsibilities gamma; loglik_out or NULL. */
PCR_API int pcr_gmm_predict(pcr_ctx* ctx, const pcr_cloud* cloud, int k, int dim, const double* means, const double* covs, const double* weights,
                            int32_t* labels_out, double* resp_out, double* loglik_out);
/* a_k(x) of deviation 1 for one point and one component on the host -- the source the kernels compile (counterpart of
 * pcr_ground_select).  PCR_E_SINGULAR: cov is not positive definite; PCR_E_INVALID: dim not 2 or 3, weight not in (0, inf).      */
PCR_API int pcr_gmm_log_density(int dim, const double* x, const double* mean, const double* cov, double weight, double* a_out);

/* --------------------------------------------------------------------- K-Means
 * class K_Means (Cluster_KMeans_GMM/compare_cluster.py:16,105: K_Means(n_clusters=...); fit(X) at :164, labels_ / predict(X) at
 * :167-170; its KMeans.py is not part of the reference tree): Lloyd's iteration on a device-resident cloud.  x_n are the cloud's
 * points (x, y, z; dim 2 uses x and y of the records and ignores z), c[k] the centres, c^0 the caller's centers0.
 *   iteration t = 1..max_iter:
 *   assign: d2(n,k) = (x-cx)^2 + (y-cy)^2 (+ (z-cz)^2) in binary64, in this direct form (never |x|^2 + |c|^2 - 2 x.c), under
 *           c^{t-1}; label_n = argmin_k d2, the lowest k on ties like np.argmin (compared with <)
 *   sums:   N_k = integer count of the points with label k (exact); S_k = sum of those points; J^{t-1} = sum_n min_k d2(n,k), the
 *           inertia of c^{t-1}
 *   update: c^t[k] = S_k / N_k where N_k > 0; an empty cluster keeps c^{t-1}[k]: it is not relocated, does not become NaN and is
 *           not an error
 *   stop:   shift_t = max_k |c^t[k] - c^{t-1}[k]|_2; shift_t <= tol ends the loop with converged = 1, otherwise it ends at
 *           t = max_iter with converged = 0.  tol = 0 is legal and means "until the assignment repeats": equal labels give
 *           bit-identical sums, hence shift = 0 exactly.
 *   After the loop one final pass under the final centres gives the labels (by caller row), the final counts and
 *   inertia = sum min d2: the numbers pcr_kmeans_fit reports (scikit-learn's labels_ and inertia_).
 *   Histories (max_iter entries each, the first result->iters are written): inertia_hist[t-1] = J^{t-1}, shift_hist[t-1] = shift_t.
 * Sums are binary64 in a fixed order without floating-point atomics: two calls on the same cloud give the same bits.  A cloud laid
 * out for a grid index (pcr_cloud_prepare: records in Morton order, id = caller row) gives its labels by caller row; its centres
 * differ by the summation order only.
 * Limits: 1 <= k <= PCR_KMEANS_MAX_K (= PCR_GMM_MAX_K: the two models seed each other), dim 2 or 3, max_iter >= 1, tol >= 0 and
 * finite, every entry of centers0 / centers finite, no NULL handle or required pointer: otherwise PCR_E_INVALID; an empty cloud:
 * PCR_E_EMPTY.  All argument checks come before anything touches the device.  centres, sums: (k,dim) row-major.             */
#define PCR_KMEANS_MAX_K 32
typedef struct pcr_kmeans_params {
    int32_t n_clusters;   /* compare_cluster.py:105 -> 2 */
    int32_t dim;          /* 2 or 3 -> 3 */
    int32_t max_iter;     /* -> 300 */
    int32_t reserved_i;
    double tol;           /* on shift_t, absolute -> 1e-4 */
    double reserved[4];
} pcr_kmeans_params;
typedef struct pcr_kmeans_result {
    int32_t iters;          /* iterations performed */
    int32_t converged;      /* shift_t <= tol fired */
    int32_t n_empty;        /* clusters without points under the final centres */
    int32_t reserved_i;
    double inertia;         /* sum min d2 under the final centres */
    double shift;           /* shift_t of the last iteration */
    double device_ms;       /* HIP events around the loop and the final pass */
    double reserved[4];
} pcr_kmeans_result;
PCR_API void pcr_kmeans_default_params(pcr_kmeans_params* p);   /* 2 clusters, dim 3, 300, 1e-4 */
/* K_Means.fit: the whole loop with its state on the device, one streaming pass per iteration plus the final one.  labels_out
 * (int32[n] by caller row), inertia_hist_out, shift_hist_out (max_iter entries each) may be NULL.                             */
PCR_API int pcr_kmeans_fit(pcr_ctx* ctx, const pcr_cloud* cloud, const pcr_kmeans_params* params, const double* centers0 /* k*dim */,
                           double* centers_out /* k*dim */, int64_t* counts_out /* k */, int32_t* labels_out, double* inertia_hist_out,
                           double* shift_hist_out, pcr_kmeans_result* result);
/* Exactly one assign + update from `centers`, for tests and for callers with their own loop: the new centres, N_k, S_k (k*dim;
 * zeros for an empty cluster), the inertia of the INPUT centres and the shift.  Every output may be NULL.                     */
PCR_API int pcr_kmeans_step(pcr_ctx* ctx, const pcr_cloud* cloud, int k, int dim, const double* centers, double* centers_out, int64_t* counts_out,
                            double* sums_out, double* inertia_out, double* shift_out);
/* K_Means.predict: labels_out[n] by caller row under `centers`; counts_out (k) and inertia_out may be NULL. */
PCR_API int pcr_kmeans_predict(pcr_ctx* ctx, const pcr_cloud* cloud, int k, int dim, const double* centers, int32_t* labels_out, int64_t* counts_out,
                               double* inertia_out);
/* A small gather by record id: xyz_out[i] = the point the caller uploaded as row rows[i], in the order asked (a row may repeat),
 * whatever the cloud's layout -- seeding from a resident or prepared cloud does not download it.  m <= 4096; a row outside
 * [0, n), m < 0 or m > 4096, a NULL pointer: PCR_E_INVALID.  Relies on the record ids being a permutation of [0, n), which every
 * cloud this library makes satisfies; a row that no record carried would come back as NaN.                                     */
PCR_API int pcr_cloud_download_rows(pcr_ctx* ctx, const pcr_cloud* cloud, const int64_t* rows /* m caller rows */, int64_t m, double* xyz_out /* m*3 */);

/* --------------------------------------------------------- spectral clustering
 * class spetral_clustering (Cluster_KMeans_GMM/spectral_clustering.py:7-46, run by compare_cluster.py:105-107) on a device-resident
 * cloud of n points.
 *   graph (:17-30): the nnk nearest OTHER rows of every row (the exact k-NN of the grid index with k = nnk + 1, the row itself dropped
 *     by id; ties by the lower row), joined to it in both directions: W is the union of the directed lists with one weight
 *     w = 1 / dist per undirected edge, dist = sqrt((dx*dx + dy*dy) + dz*dz) as pcr_knn reports it.  W is kept as a CSR whose
 *     columns ascend within a row; a row's length is not bounded by 2 nnk.  The degree d_i is the sum of row i's weights in column
 *     order.  Two distinct rows at distance 0 (the reference's weight is infinite) end the call with PCR_E_SINGULAR,
 *     bad_row = the lowest such caller row, nothing written.
 *   eigenvectors (:32-39): the m = n_clusters smallest eigenpairs of the Laplacian, from the largest eigenvalues theta of a symmetric
 *     operator B with spectrum in [-1, 1]:
 *       normalized:     B = D^-1/2 W D^-1/2,          lambda = 1 - theta           (scale 1)
 *       not normalized: B = I - (D - W) / d_max,      lambda = d_max (1 - theta)   (scale d_max = the largest degree)
 *     Stated deviation: the reference calls LA.eig on the non-symmetric D^-1 L, which is similar to I - D^-1/2 W D^-1/2; the symmetric
 *     form has real eigenpairs always, where LA.eig returns complex pairs on some inputs and the reference then raises.
 *     n > 64: Chebyshev-filtered subspace iteration on a block of p = m + 8 vectors (binary64, row-major n x p).  Start: a hash of
 *     (caller row, column) to (-1, 1), no RNG.  Outer iteration: the degree-20 Chebyshev filter that damps [-1, cut] (cut = the smallest
 *     Ritz value of the previous iteration, 0 at first), the three-term recurrence fused into the sparse product; columns scaled to
 *     unit norm and Cholesky-QR twice; Rayleigh-Ritz with a cyclic Jacobi solve of the p x p matrix; residuals
 *     r_j = |B u_j - theta_j u_j|_2.  It stops with converged = 1 when r_j <= 2 tol for all j < m, else after max_iter iterations with
 *     converged = 0 (eigenvalues, residuals and embedding of the last iterate are still returned).  A Cholesky pivot that is not
 *     positive or not finite: PCR_E_SINGULAR with bad_row = -1.  spmm counts the sparse products (21 per outer iteration).
 *     n <= 64: the dense n x n operator and the same Jacobi routine on the host (iters = 0, spmm = 0, converged = 1).
 *     embedding column j (n x m, row-major, by caller row): normalized: D^-1/2 u_j (the eigenvector of D^-1 L), else u_j; scaled to
 *     unit 2-norm; sign: the entry of largest magnitude is positive, the lowest caller row on ties.  Inside a repeated eigenvalue
 *     only the span is defined, as in the reference.
 *   K-Means (:43) on the rows of the embedding under the rules of pcr_kmeans_fit above (direct-form squared distances summed in
 *     column order, the lowest cluster on ties, an empty cluster keeps its centre, stop on shift <= kmeans_tol, a final labelling
 *     pass).  Seeds are rows of the embedding: the caller's seed_rows, or maximin from caller row 0 (seed j = the row with the largest
 *     minimum squared distance to the seeds before it, the lowest row on ties).  Cluster j is the one seeded by seed j.  (The
 *     reference calls scikit-learn's KMeans with k-means++ and restarts on the global RNG, which cannot be pinned.)
 * Every sum runs in a fixed order without floating-point atomics: two calls on the same cloud give the same bits.  Rows and columns
 * are kept in the Morton order of the index built for the k-NN; everything handed to the caller is by caller row.
 * Limits, all checked before anything touches the device: 1 <= n_clusters <= PCR_SPECTRAL_MAX_K, 1 <= nnk <= PCR_SPECTRAL_MAX_NNK,
 * max_iter >= 1, kmeans_max_iter >= 1, tol finite and > 0, kmeans_tol finite and >= 0, no NULL handle or required pointer: otherwise
 * PCR_E_INVALID; then an empty cloud: PCR_E_EMPTY; then n < nnk + 2 (the reference raises IndexError), n < n_clusters, a seed row
 * outside [0, n) or repeated: PCR_E_INVALID.                                                                                      */
#define PCR_SPECTRAL_MAX_K 8
#define PCR_SPECTRAL_MAX_NNK 15
typedef struct pcr_spectral_params {
    int32_t n_clusters;        /* -> 2 */
    int32_t nnk;               /* -> 7 */
    int32_t normalized;        /* -> 1 */
    int32_t max_iter;          /* outer iterations of the eigensolver -> 200 */
    int32_t kmeans_max_iter;   /* -> 300 */
    int32_t reserved_i;
    double tol;                /* on the residuals, absolute: r_j <= 2 tol -> 1e-8 */
    double kmeans_tol;         /* -> 1e-4 */
    double reserved[4];
} pcr_spectral_params;
typedef struct pcr_spectral_result {
    int32_t iters;             /* outer iterations performed */
    int32_t converged;
    int32_t spmm;              /* sparse products performed */
    int32_t max_degree;        /* the longest row of W */
    int32_t bad_row;           /* PCR_E_SINGULAR from the graph: the lowest row with another row at distance 0; -1 otherwise */
    int32_t kmeans_iters;
    int32_t kmeans_converged;
    int32_t n_empty;           /* clusters without points under the final centres */
    int64_t n_edges;           /* undirected edges of W */
    double eigenvalues[8];     /* lambda_j, j < n_clusters, ascending */
    double residuals[8];       /* r_j of the operator B */
    double next_eigenvalue;    /* lambda_{m+1} (a Ritz value of the guard block): the gap behind the last wanted one; NaN when n = m */
    double inertia;            /* of the K-Means on the embedding, under the final centres */
    double graph_ms;           /* HIP events: index, k-NN, CSR */
    double solver_ms;          /* operator, subspace iteration, embedding */
    double kmeans_ms;          /* seeds, Lloyd's loop, final pass */
    double reserved[4];
} pcr_spectral_result;
PCR_API void pcr_spectral_default_params(pcr_spectral_params* p);   /* 2, 7, 1, 200, 300, 1e-8, 1e-4 */
/* The graph alone, by caller row, in two passes like pcr_radius: with indices_out == NULL it fills indptr_out (n + 1 entries) only;
 * with indices_out and weights_out (indptr_out[n] entries each, columns ascending) it fills all three.  bad_row_out (or NULL): -1, or
 * the row of PCR_E_SINGULAR.                                                                                                      */
PCR_API int pcr_knn_graph(pcr_ctx* ctx, const pcr_cloud* cloud, int nnk, int64_t* indptr_out /* n+1 */, int32_t* indices_out, double* weights_out,
                          int32_t* bad_row_out);
/* Graph and eigenvectors: embedding_out (n*m, by caller row); result's K-Means fields stay zero. */
PCR_API int pcr_spectral_embed(pcr_ctx* ctx, const pcr_cloud* cloud, const pcr_spectral_params* params, double* embedding_out /* n*m */,
                               pcr_spectral_result* result);
/* spetral_clustering.fit: labels_out (int32[n] by caller row).  seed_rows (k caller rows) may be NULL: maximin.  embedding_out (n*m),
 * centers_out (k*m, rows of the embedding space) and seed_rows_out (k, the seeds used) may be NULL.                               */
PCR_API int pcr_spectral_fit(pcr_ctx* ctx, const pcr_cloud* cloud, const pcr_spectral_params* params, const int64_t* seed_rows /* k or NULL */,
                             int32_t* labels_out, double* embedding_out /* or NULL */, double* centers_out /* k*m or NULL */,
                             int64_t* seed_rows_out /* k or NULL */, pcr_spectral_result* result);
/* The cyclic Jacobi eigen-solve the kernels compile, on the host: A symmetric n x n row-major (not modified), 1 <= n <= 64 (else
 * PCR_E_INVALID); eigvals_out (n) ascending, eigvecs_out (n x n row-major) column j = the unit eigenvector of eigvals_out[j].      */
PCR_API int pcr_sym_eig_jacobi(int n, const double* A, double* eigvals_out, double* eigvecs_out);

/* ------------------------------------------- PointNet++ set-abstraction ops
 * The op library of the reference's classifier (Final_Project/pointnet2_ops_lib/pointnet2_ops/pointnet2_utils.py: furthest_point_sample
 * :65, gather_operation :101, three_nn :136, three_interpolate :191, grouping_operation :240, ball_query :276), whose native half
 * exists only as CUDA.  Unlike the rest of this header these functions work on the CALLER'S device memory:
 *   - every array is a device pointer on the current device, C-contiguous, binary32 data and int32 indices, laid out as the
 *     reference lays them out (shapes are given beside each parameter);
 *   - `stream` is a hipStream_t (NULL: the null stream); the kernels are enqueued there and the call returns at once;
 *   - no pcr_ctx, no allocation, no host synchronisation; workspaces are the caller's;
 *   - PCR_OK, PCR_E_INVALID (a negative size, no input points or a NULL pointer where the output is not empty, a radius that is
 *     not finite, more than 2^31 - 1 blocks) or PCR_E_HIP (the launch failed).  b == 0 or any other size that makes the output
 *     empty: PCR_OK, nothing is launched.
 * Arithmetic is binary32 without contraction, in the order written below, so a NumPy float32 restatement gives the same bits.
 * Inputs must be finite and every entry of an index array must lie inside the array it addresses; neither is validated.
 *
 * Furthest point sampling, per cloud of n points, m picks:
 *   eligible(k): ((x*x + y*y) + z*z of point k, binary32), widened to binary64, > 1e-3.  A point that is not eligible is never
 *                updated and never chosen (padding rows at the origin).
 *   temp[k] = 1e10f.  pick 0 = index 0, whether eligible or not.
 *   pick j >= 1: p = the point of pick j-1; for every eligible k: d = ((dx*dx) + (dy*dy)) + (dz*dz) with dx = x_k - x_p, ...;
 *                temp[k] = min(d, temp[k]); the pick is the eligible k of the largest temp[k], the LOWEST k among equals;
 *                no eligible point at all: the pick is 0.
 *   m > n is legal (picks repeat).  The tie rule is a rule of its own: in the reference the winner among equal distances depends on
 *   how many threads its block happens to have, which no caller can rely on.
 *   temp is a workspace of b*n floats; its contents afterwards are unspecified.
 * Ball query: r = radius as binary32, r2 = r*r in binary32; d2 = ((dx*dx) + (dy*dy)) + (dz*dz).  A centre's row holds, in increasing
 *   index order, the first nsample points with d2 < r2 (strictly); a centre with fewer hits fills the rest of its row with its
 *   first hit; a centre without a hit gets a row of zeros.
 * three_nn: for every unknown point the three smallest d (same form) over the known points, ascending, kept by insertion with a
 *   strict <: of equal distances the earlier index stays ahead.  m < 3: the empty slots report +inf and index 0.  dist2_out holds
 *   SQUARED distances.
 * three_interpolate: out[b,c,i] = (p[idx0]*w0 + p[idx1]*w1) + p[idx2]*w2 with p = points[b,c,:], idx and w from row (b,i).
 * gather_points: out[b,c,j] = points[b,c,idx[b,j]].  group_points: out[b,c,j,s] = points[b,c,idx[b,j,s]].                       */
PCR_API int pcr_pn2_furthest_point_sampling(void* stream, int b, int n, int m, const float* xyz /* b,n,3 */, float* temp /* b,n workspace */,
                                            int32_t* idx_out /* b,m */);
PCR_API int pcr_pn2_ball_query(void* stream, int b, int n, int m, float radius, int nsample, const float* new_xyz /* b,m,3 */,
                               const float* xyz /* b,n,3 */, int32_t* idx_out /* b,m,nsample */);
PCR_API int pcr_pn2_three_nn(void* stream, int b, int n, int m, const float* unknown /* b,n,3 */, const float* known /* b,m,3 */,
                             float* dist2_out /* b,n,3 */, int32_t* idx_out /* b,n,3 */);
PCR_API int pcr_pn2_three_interpolate(void* stream, int b, int c, int m, int n, const float* points /* b,c,m */, const int32_t* idx /* b,n,3 */,
                                      const float* weight /* b,n,3 */, float* out /* b,c,n */);
PCR_API int pcr_pn2_gather_points(void* stream, int b, int c, int n, int npoints, const float* points /* b,c,n */, const int32_t* idx /* b,npoints */,
                                  float* out /* b,c,npoints */);
PCR_API int pcr_pn2_group_points(void* stream, int b, int c, int n, int npoints, int nsample, const float* points /* b,c,n */,
                                 const int32_t* idx /* b,npoints,nsample */, float* out /* b,c,npoints,nsample */);

/* ------------------------------------------- PointNet++ gradients
 * The gradients of gather, group and three_interpolate with respect to their features (the reference's gather_points_grad,
 * group_points_grad and three_interpolate_grad, called from pointnet2_utils.py:93-99, :217-237 and :164-189; its kernels add with
 * atomicAdd, in no order).  Same calling rules as the ops above: caller's device memory, caller's stream, no context, no allocation,
 * no host synchronisation.  All three are the transpose of a gather along the last axis.  With k slots per cloud and
 * idx[b, slot] in [0, n):
 *   grad_points[b, c, i] = sum of term[b, c, slot] over the slots with idx[b, slot] == i, in ASCENDING slot order: the accumulator
 *   starts at +0.0f and takes one rounded binary32 addition per term; a point that no slot names gets +0.0f.
 *   gather:            k = npoints,          term = grad_out[b, c, slot]
 *   group:             k = npoints*nsample,  slot = j*nsample + s,  term = grad_out[b, c, j, s]
 *   three_interpolate: k = 3*n,              slot = 3*j + kk,       term = grad_out[b, c, j] * weight[b, j, kk], rounded once (no
 *                      fused multiply-add), then added; here the points are the m known ones.
 * This is what np.add.at(out, idx, term) does on a float32 array, so the result is the same bits on every run and on the host.  No
 * floating-point atomics are used.  Infinities follow the same additions; the sign and payload of a NaN they produce are not
 * part of the contract.
 *
 * The inverse index says, per point, which slots name it: start (b, n + 1) and slots (b, k), point i of cloud bi owning
 * slots[bi, start[bi, i] .. start[bi, i+1]) in ascending order; start[bi, 0] = 0, start[bi, n] = k.  It is a function of idx alone,
 * is built once per index tensor (pcr_pn2_inverse_index, a stable radix sort of the pairs (bi*n + idx, slot) on the caller's
 * stream) and serves every channel and every tensor that was gathered with that idx.  Its workspace of
 * pcr_pn2_inverse_index_bytes(b, n, k) bytes is the caller's, 256-byte aligned, and free again once the stream has passed the
 * call.  The query returns the size (0 for an empty problem) or a negative PCR_E_* code.
 * Status: PCR_E_INVALID for a negative size, a NULL pointer where data is needed, n == 0 with slots to place, a workspace that is
 * misaligned or too small; PCR_E_UNSUPPORTED for b*n > 2^32 (the sort's keys), k > 2^31 - 1, or more than 65 535 clouds or channel
 * tiles; PCR_E_HIP for a failed launch.  b == 0, c == 0 or no points: PCR_OK, nothing is launched.  k == 0 with points: start is
 * zeroed, grad_points is zeroed.  Entries of idx are assumed in range, as for the forward ops.                                   */
PCR_API long long pcr_pn2_inverse_index_bytes(int b, int n, int k);
PCR_API int pcr_pn2_inverse_index(void* stream, int b, int n, int k, const int32_t* idx /* b,k */, void* workspace, long long workspace_bytes,
                                  int32_t* start_out /* b,n+1 */, int32_t* slots_out /* b,k */);
PCR_API int pcr_pn2_gather_points_grad(void* stream, int b, int c, int n, int npoints, const float* grad_out /* b,c,npoints */,
                                       const int32_t* start /* b,n+1 */, const int32_t* slots /* b,npoints */, float* grad_points /* b,c,n */);
PCR_API int pcr_pn2_group_points_grad(void* stream, int b, int c, int n, int npoints, int nsample, const float* grad_out /* b,c,npoints,nsample */,
                                      const int32_t* start /* b,n+1 */, const int32_t* slots /* b,npoints*nsample */, float* grad_points /* b,c,n */);
PCR_API int pcr_pn2_three_interpolate_grad(void* stream, int b, int c, int n, int m, const float* grad_out /* b,c,n */,
                                           const int32_t* start /* b,m+1 */, const int32_t* slots /* b,3*n */, const float* weight /* b,n,3 */,
                                           float* grad_points /* b,c,m */);

/* Set abstraction for inference, fused: gather, shared MLP (batch norm folded into the weights by the caller), ReLU and the maximum
 * over the ball in one kernel; the grouped tensor (b, C, m, nsample) is never stored.  Same calling rules as the ops above.  `widths`,
 * `weights` and `biases` are HOST arrays of n_layers entries (read during the call); weights[l] and biases[l] are device pointers,
 * layer l's matrix (widths[l], K_l) row-major with K_l = widths[l-1] (K_0 below) and its bias (widths[l]).  `feats` is POINT-major
 * (b, n, c_feat), so a row's gather is one contiguous read; NULL iff c_feat == 0.  Element (bi, j, ci) of the result is
 * out[bi*out_batch_stride + j*m + ci]: with out_batch_stride = (sum of all scales' widths) * m every scale of a multi-scale module
 * writes straight into its channel range of the concatenated (b, sum C, m) tensor.
 * Contract.  All arithmetic is binary32, no contraction in the VALU parts.
 *   - The row for (centre ci, sample s) is built from p = idx[bi, ci, s].  With use_xyz its first three entries are
 *     xyz[bi, p, :] - new_xyz[bi, ci, :]; then follow feats[bi, p, 0:c_feat].  K_0 = 3*use_xyz + c_feat, which must be at least 1.
 *   - Layer l computes acc = bias_l[j], then for k = 0 .. K_l-1 in ascending order acc = fmaf(x[k], W_l[j,k], acc), then
 *     y[j] = acc > 0 ? acc : +0.
 *   - out[bi, j, ci] = max over s of y_last[j].  Every y is at least +0, so the maximum has no sign or NaN cases on finite input.
 *     Inputs must be finite and indices in range; neither is validated, as for the other ops.
 *   - Padding rows never enter the maximum: a tile row that stands for no (ci, s) pair is a copy of a real row of the same unit and
 *     is masked out of the pooling; it is never a row of zeros, whose relu(bias) could win the maximum.
 *   - There is no cross-workgroup floating-point accumulation; in this implementation no two workgroups share a centre at all (a
 *     workgroup owns whole centres), so every (bi, j, ci) is stored once, `out` needs no zeroing and elements outside the addressed
 *     ones are not touched.  The result is bitwise repeatable.
 *   - PCR_OK for a normal call; PCR_E_INVALID for a negative size, nsample < 1 or n < 1 with a non-empty output, K_0 < 1,
 *     n_layers < 1, a width below 1, or a NULL pointer where data is needed; PCR_E_UNSUPPORTED, before any launch, for a shape the
 *     kernel declines; PCR_E_HIP for a failed launch.  An empty output (b == 0 or m == 0) returns PCR_OK and launches nothing.
 *   - Supported: 1 to PCR_PN2_SA_MAX_LAYERS layers, every width at most PCR_PN2_SA_MAX_WIDTH, K_0 at most PCR_PN2_SA_MAX_K0, at
 *     most 2^31 - 1 workgroups.  The width limit is the on-chip budget: a workgroup keeps a 64-row tile of one layer's activations
 *     in LDS (64 x 257 floats) beside a 32-column stage of the weights (256 x 33) and of the gathered rows (64 x 33), 107 KiB of
 *     160, and the tile's accumulators in registers (64 per lane at width 256).  K_0 is streamed 32 columns at a time and is not
 *     bounded by LDS; 1024 is the range that is tested.  This covers every module of the reference's classifiers that has centres
 *     (K_0 up to 323, widths up to 256).                                                                                          */
#define PCR_PN2_SA_MAX_LAYERS 3
#define PCR_PN2_SA_MAX_WIDTH 256
#define PCR_PN2_SA_MAX_K0 1024
PCR_API int pcr_pn2_sa_mlp_max(void* stream, int b, int n, int m, int nsample, int c_feat, int use_xyz, const float* xyz /* b,n,3 */,
                               const float* new_xyz /* b,m,3 */, const float* feats /* b,n,c_feat or NULL */,
                               const int32_t* idx /* b,m,nsample */, int n_layers, const int* widths /* host, n_layers */,
                               const float* const* weights /* host, n_layers device pointers */,
                               const float* const* biases /* host, n_layers device pointers */, float* out, long long out_batch_stride);

/* Feature propagation for inference, fused: the three-point interpolation of the known points' features, the concatenation with the
 * points' own (skip) features and the per-point shared MLP (batch norm folded into the weights by the caller) in one kernel; neither
 * the interpolated tensor nor the (b, c_known + c_skip, n) concatenation nor any layer's intermediate is stored.  Same calling rules
 * as pcr_pn2_sa_mlp_max: the caller's device memory and stream, no context, no allocation, no wait; `widths`, `weights` and `biases`
 * are HOST arrays of n_layers entries read during the call, weights[l] (widths[l], K_l) row-major and biases[l] (widths[l]) device
 * pointers, K_l = widths[l-1].  The neighbour search is not part of it: idx and weight are pcr_pn2_three_nn's indices and the
 * caller's normalised inverse distances, as for pcr_pn2_three_interpolate.  Both feature tensors are POINT-major.
 * Contract.  All arithmetic is binary32, no contraction in the VALU parts.
 *   - Row layout.  The row of point (bi, i) has K_0 = c_known + c_skip >= 1 entries.  For k < c_known:
 *     ((p0*w0) + (p1*w1)) + (p2*w2) with pj = known_feats[bi, idx[bi,i,j], k] and wj = weight[bi,i,j], the expression and order of
 *     pcr_pn2_three_interpolate.  Then follow skip_feats[bi, i, 0:c_skip], without padding between the two parts.  c_known == 0 is
 *     legal and makes the call a plain per-point shared MLP (known_feats, idx and weight are then not read and may be NULL).
 *   - Layer l computes acc = bias_l[j], then for k = 0 .. K_l-1 in ascending order acc = fmaf(x[k], W_l[j,k], acc): one chain per
 *     output, no split over k, exactly as for pcr_pn2_sa_mlp_max.  After every layer but the last, and after the last one when
 *     relu_last != 0: y[j] = acc > 0 ? acc : +0.  With relu_last == 0 the last layer stores acc + (+0.0f): an accumulator of -0 is
 *     stored as +0, for every K.
 *   - out[bi, j, i] (b, widths[n_layers-1], n) is stored once: no two workgroups share a row, there are no atomics, `out` needs no
 *     zeroing and elements outside the addressed ones are not touched.  The result is bitwise repeatable.  A tile row that stands
 *     for no point is a copy of the last real row and is never stored.
 *   - Inputs must be finite and indices in range; neither is validated, as for the other ops.
 *   - PCR_OK for a normal call; PCR_E_INVALID for a negative size, K_0 < 1, n_layers < 1, a width below 1, m < 1 with c_known > 0
 *     and a non-empty output, or a NULL pointer where data is needed; PCR_E_UNSUPPORTED, before any launch, for a shape the kernel
 *     declines; PCR_E_HIP for a failed launch.  An empty output (b == 0 or n == 0) returns PCR_OK and launches nothing.
 *   - Supported: 1 to PCR_PN2_FP_MAX_LAYERS layers, every width at most PCR_PN2_FP_MAX_WIDTH, K_0 at most PCR_PN2_FP_MAX_K0, at most
 *     2^31 - 1 workgroups of 64 rows.  The on-chip budget is the set-abstraction kernel's: a 64-row tile of one layer's activations
 *     in LDS (64 x 257 floats) beside a 32-column stage of the weights (256 x 33) and of the rows (64 x 33) and 3 KiB of per-row
 *     words, 109 KiB of 160, and the tile's accumulators in registers.  K_0 is streamed 32 columns at a time.  This covers every
 *     decoder module and the head of the reference's segmentation networks except the two deepest modules of the multi-scale one
 *     (widths 512).                                                                                                               */
#define PCR_PN2_FP_MAX_LAYERS 3
#define PCR_PN2_FP_MAX_WIDTH 256
#define PCR_PN2_FP_MAX_K0 1024
PCR_API int pcr_pn2_fp_mlp(void* stream, int b, int n, int m, int c_known, int c_skip,
                           const float* known_feats /* b,m,c_known point-major; NULL iff c_known == 0 */,
                           const int32_t* idx /* b,n,3; NULL iff c_known == 0 */, const float* weight /* b,n,3; NULL iff c_known == 0 */,
                           const float* skip_feats /* b,n,c_skip point-major; NULL iff c_skip == 0 */, int n_layers,
                           const int* widths /* host, n_layers */, const float* const* weights /* host, n_layers device pointers */,
                           const float* const* biases /* host, n_layers device pointers */, int relu_last,
                           float* out /* b, widths[n_layers-1], n */);

/* ----------------------------------------------------------- object batches
 * The stage between DBSCAN's labels and the classifier's input: `preprocess` of Final_Project/scripts/detect.py:269-354, whose
 * resampling step also builds the training set (generating-training-set.py:186-194).  All arithmetic is binary64 on the stored
 * coordinates, in the order written here, without contraction, so that NumPy / SciPy give the same bits.
 *
 * pcr_objects_build groups the rows of a device-resident cloud by labels[row] (n entries BY CALLER ROW, whatever the order of the
 * records on the device: pcr_cloud_reordered).  A label < 0 is noise and belongs to no object; a label >= n_objects: PCR_E_INVALID
 * (checked before any launch); an id without rows is an object of count 0.  Within an object the rows stay in ascending caller row
 * (points[object_ids == o], detect.py:295).  Empty cloud: PCR_E_EMPTY; more than 2^31 - 1 rows: PCR_E_UNSUPPORTED.  The handle keeps
 * the grouped records and the statistics on the device and does not refer to the cloud afterwards.
 *   offsets[n_objects + 1]: object o owns [offsets[o], offsets[o+1]) of the grouped order; offsets[n_objects] = m, the labelled rows.
 *   rows[m]: the caller rows in the grouped order.
 *   stats, each output optional: count[o] = offsets[o+1] - offsets[o] ((object_ids == o).sum(), detect.py:286);
 *     mean[3o + a] = (((c_0 + c_1) + c_2) + ...) / (double)count over the object's rows in ascending order (np.mean(axis=0),
 *     detect.py:290 and :312); bmin / bmax the axis-aligned box (detect.py:244).  An object of count 0: mean NaN (0.0 / 0.0, like
 *     np.mean of nothing), bmin +inf, bmax -inf.
 * pcr_objects_select, on the host (no context; counterpart of pcr_ground_select): keep[o] = count[o] > min_count (detect.py:286 with
 *   min_count = 4: five rows are kept) and sqrt(mx*mx + my*my) <= max_radius (detect.py:291 skips on >, so a centre exactly on the
 *   radius is kept).  A NaN centre is dropped: the reference's comparison would let it pass and np.random.choice then refuses its
 *   weights.
 * pcr_objects_weights: weights[k] for every grouped row k, unnormalised (detect.py:299-301):
 *     w_i = (((d_i0 + d_i1) + d_i2) + ... + d_i,n-1) / (double)n,  j ascending over ALL n rows of i's object, d_ii = +0.0 included,
 *     d_ij = sqrt(((dx*dx) + dy*dy) + dz*dz), dx = x_i - x_j, ...                 (pdist 'euclidean', then the column mean)
 *   keep (n_objects flags, or NULL = every object): rows of an object that is not kept get 0.  The n x n matrix is never stored; a
 *   wave owns 64 rows i and stages the rows j through on-chip memory PCR_OBJECTS_TILE at a time.  `weights /= weights.sum()`
 *   (detect.py:302) is NumPy's pairwise sum and stays with the caller.
 * pcr_objects_pack_f32 fills the classifier's batch (detect.py:311-318, then .float()) at a DEVICE address of the context's device:
 *   slot s (of b) shows object slot_object[s]; local_idx[s*S + k] is a position within that object in ascending row order, which is
 *   what np.random.choice(np.arange(N), ...) returns (detect.py:304).  out[s][k] = { (float)(x - mean_x), (float)(y - mean_y),
 *   (float)(z - mean_z), (float)nx, (float)ny, (float)nz }: the subtraction in binary64 with the mean of pcr_objects_stats, then
 *   rounded to nearest; normals (n x 3 binary64 on the host, BY CALLER ROW) may be NULL, and the rows are then 3 floats.  C-contiguous
 *   (b, S, 6) or (b, S, 3).  The call returns after the context's stream has drained: the caller's framework may read the tensor at
 *   once (it must have finished its own earlier work on that memory).  PCR_E_INVALID, before any launch: an object outside
 *   [0, n_objects), an index outside [0, count), a NULL array.  b == 0 or S == 0: PCR_OK, nothing is launched.                       */
#define PCR_OBJECTS_TILE 128
typedef struct pcr_objects pcr_objects;
PCR_API int pcr_objects_build(pcr_ctx* ctx, const pcr_cloud* cloud, const int32_t* labels /* n, by caller row */, int32_t n_objects, pcr_objects** out);
PCR_API int pcr_objects_free(pcr_ctx* ctx, pcr_objects* objs);
PCR_API int pcr_objects_offsets(const pcr_objects* objs, int64_t* offsets /* n_objects + 1 */);
PCR_API int pcr_objects_rows(pcr_ctx* ctx, const pcr_objects* objs, int32_t* rows /* m */);
PCR_API int pcr_objects_stats(pcr_ctx* ctx, const pcr_objects* objs, int64_t* count /* n_objects */, double* mean /* n_objects*3 */, double* bmin, double* bmax);
PCR_API int pcr_objects_select(const int64_t* count, const double* mean, int32_t n_objects, int64_t min_count, double max_radius, uint8_t* keep /* n_objects */);
PCR_API int pcr_objects_weights(pcr_ctx* ctx, const pcr_objects* objs, const uint8_t* keep /* n_objects or NULL */, double* weights /* m */);
PCR_API int pcr_objects_pack_f32(pcr_ctx* ctx, const pcr_objects* objs, const double* normals /* n*3 or NULL */, const int32_t* slot_object /* b */,
                                 const int64_t* local_idx /* b*S */, int64_t b, int64_t S, void* out_device /* b*S*(6 or 3) floats */);

/* -------------------------------------------------------------- KITTI boxes
 * The per-object part of `to_kitti_eval_format` (Final_Project/scripts/detect.py:106-163 with get_orientation_in_camera_frame,
 * detect.py:37-54, and transform_coords_utils.py): the 2-D pixel box, the camera-frame centre, the PCA heading on the x-z plane and
 * the extents in the heading-aligned object frame, for every object of a pcr_objects handle in ONE launch (one wave per object).
 * The calibration matrices are row-major with read_calib's shapes (extract.py:49-84): R0_rect 3x3, Tr_velo_to_cam = T 3x4, P2 = P 3x4.
 *
 * Everything is binary64 in exactly this order, without contraction or atomics; nothing depends on arrival order.  Per row (x, y, z):
 *   u_i = ((T[i][0]*x + T[i][1]*y) + T[i][2]*z) + T[i][3]                   unrectified camera frame
 *   X_i = (R0[i][0]*u_0 + R0[i][1]*u_1) + R0[i][2]*u_2                      rectified camera frame
 *   q_i = ((P[i][0]*X_0 + P[i][1]*X_1) + P[i][2]*X_2) + P[i][3],  px = q_0/q_2, py = q_1/q_2   (no special case for q_2 <= 0: the
 *     reference has none; a NaN pixel coordinate takes no part in the pixel box)
 * The object sum S over the n rows of an object in grouped order (ascending caller row): p_l, l = 0 .. 63, starts from +0.0 and
 *   adds rows l, l + 64, ... ascending; then p_l += p_{l+s} for every l < s, for s = 32, 16, 8, 4, 2, 1; the sum is p_0.  This order
 *   belongs to the ABI, not to the launch shape.
 *   ctr_i = S(X_i) / (double)n;  d_i = X_i - ctr_i;
 *   a = S(d_0*d_0) / n, b = S(d_0*d_2) / n, c = S(d_2*d_2) / n       (np.cov(bias=True) of the centred rows without its second
 *     centring, whose effect is of the order of one rounding of the centre)
 *   (cs, sn) = pcr_kitti_direction(a, b, c), below;  ry = atan2(sn, cs) is the CALLER's: no transcendental runs on the device.
 *   object frame (detect.py:135-148 with cos(-ry) = cs, sin(-ry) = -sn):  xo = cs*d_0 - (-sn)*d_2, yo = d_1, zo = (-sn)*d_0 + cs*d_2
 *   extent per axis = max - min, the max taken as -(min of the negated values).
 * pcr_kitti_direction (host, no context; the kernel compiles the same source): with h = (a - c)*0.5,
 *   b == 0:            (1, -0.0) if h > 0, else (0, -1)
 *   b != 0, h >= 0:    e = (h + r, b)       with r = sqrt(h*h + b*b)
 *   b != 0, h <  0:    e = (-b, r - h)
 *   and (cs, sn) = e / sqrt(e0*e0 + e1*e1) in the last two cases.  This is what detect.py:47-54 returns with NumPy 2.2 / OpenBLAS
 *   0.3.29 (LAPACK dgeev on a symmetric 2x2): the reference reads ROW 0 of the matrix of eigenvectors, sorted by descending
 *   eigenvalue, so for h < 0 its angle is not the principal axis.  PCR_E_INVALID: cs or sn NULL.
 * boxes[16*o + ...]: 0..3 left, top, right, bottom (min / max of px, py); 4..6 height = extent of yo, width = extent of xo, length =
 *   extent of zo; 7..9 ctr; 10..11 cs, sn; 12..14 a, b, c; 15 (double)count.  An object of count 0 or with keep[o] == 0: entries
 *   0..14 are NaN, entry 15 is the count, and no pass runs for it.  Count 1: extents +0.0, direction (0, -1).
 * An object of at most PCR_KITTI_LDS_ROWS rows keeps its camera-frame rows on chip between the three passes; a larger one computes
 *   them again from the grouped records -- the same operations, the same bits.
 * PCR_E_INVALID, before any launch: objs, calib or boxes NULL, a calibration entry (R0_rect, Tr_velo_to_cam, P2) that is not finite.
 * No objects: PCR_OK, nothing is launched.  The call returns after the context's stream has drained.                              */
typedef struct pcr_kitti_calib { double R0_rect[9]; double Tr_velo_to_cam[12]; double P2[12]; double reserved[4]; } pcr_kitti_calib;
#define PCR_KITTI_BOX_DOUBLES 16
#define PCR_KITTI_LDS_ROWS 512
PCR_API int pcr_kitti_direction(double a, double b, double c, double* cs, double* sn);
PCR_API int pcr_objects_kitti_boxes(pcr_ctx* ctx, const pcr_objects* objs, const pcr_kitti_calib* calib, const uint8_t* keep /* n_objects or NULL */,
                                    double* boxes /* n_objects*16 */);

/* -------------------------------------------------------------- label match
 * Training-set extraction: the per-label part of `process_sample` (Final_Project/scripts/extract.py:506-574) for ALL the KITTI 3-D
 * labels of a frame in ONE launch (one workgroup per label) over the grouped rows of a pcr_objects handle: the rows in the label's
 * sphere (search_radius_vector_3d, :522), moved into the label's object frame (transform_from_velo_to_obj, :116-164), those inside the
 * label's box vote for their object (filter_by_bouding_box, :166-201), and the in-sphere rows of the winning object are the sample
 * (:552-574).
 *
 * labels[16*l + ...]: 0..2 vx, vy, vz, the sphere centre in the Velodyne frame (read_label's value, `+ height/2` already added);
 *   3 radius;  4..6 cx, cy, cz, the centre in the rectified camera frame;  7, 8 cos(ry), sin(ry) -- the CALLER takes them: no
 *   transcendental runs on the device, as for the boxes;  9..11 length, height, width;  12..15 reserved, must be 0.
 * Per grouped row (x, y, z), everything binary64 in exactly this order, without contraction:
 *   dx = x - vx, dy = y - vy, dz = z - vz;   in_sphere = (dx*dx + dy*dy) + dz*dz <= radius*radius
 *     (the library's boundary rule, as in pcr_iss and pcr_dbscan: a row exactly on the sphere is inside.  What Open3D / FLANN do at
 *     exact equality is UNPINNED: their squared distance is accumulated in another order.)
 *   u_i, X_i as written for the KITTI boxes above (Tr_velo_to_cam, then R0_rect; P2 is not used);   e_i = X_i - c_i
 *   xo = cos*e_0 - sin*e_2;   yo = e_1 + height/2;   zo = sin*e_0 + cos*e_2
 *     (R_obj_to_cam.T . e of extract.py:152-162 with its exact-zero terms dropped, then :541)
 *   in_box = -length/2 <= xo <= length/2 && -height/2 <= yo <= height/2 && -width/2 <= zo <= width/2   (both faces inclusive,
 *     extract.py:184-190)
 * Per label:
 *   k = the rows with in_sphere, over all objects;   votes[o] = the rows of object o with in_sphere && in_box;
 *   winner = the LOWEST o with the largest votes[o] > 0 (np.unique ascends and max(..., key) keeps the first maximum, :196-199);
 *     -1 when no row is in the box (`return None`, :192);
 *   the selected rows = the rows of the winner with in_sphere -- not in_box (:552);  n_sel their count;
 *   centre_a = S(selected coordinate a) / (double)n_sel, S the object sum of the KITTI boxes restricted to the selected rows:
 *     position p = 0 .. count-1 within the winner belongs to lane p % 64; p_l starts from +0.0 and adds its SELECTED rows in
 *     ascending p (a skipped row adds nothing); then p_l += p_{l+s} for every l < s, s = 32, 16, 8, 4, 2, 1; the sum is p_0.  This
 *     order belongs to the ABI, not to the launch shape.
 * result[8*l + ...]: 0 k;  1 winner or -1.0;  2 votes[winner];  3 n_sel;  4..6 centre;  7 +0.0.  Without a winner entries 2 and 3 are
 *   0.0 and entries 4..6 are NaN.
 * sel_bits (may be NULL): bit p % 64 of word l*words + p/64 is set iff position p of the winner is selected; every word of the
 *   L*words block is written, those beyond the winner's count (all of them without a winner) with zero.  `words` must be at least
 *   ceil(max object count / 64): PCR_E_INVALID otherwise.
 * An object whose stored box (pcr_objects_stats) cannot meet the sphere is not read; the test is made in the arithmetic of in_sphere
 *   itself, whose every step is monotone, so it never changes k, the votes or any bit of the output.
 * PCR_E_INVALID, before any launch: objs, calib, labels (with L > 0) or result NULL; a calibration entry (R0_rect, Tr_velo_to_cam, P2: the
 *   struct is checked as for the boxes) or a label entry 0..11 that is not finite; a negative radius or dimension; a reserved entry that is not zero; L < 0.  L == 0: PCR_OK.  A handle
 *   without labelled rows: PCR_OK, every label gets k = 0, winner = -1, and nothing is launched.  The call returns after the
 *   context's stream has drained.                                                                                               */
#define PCR_LABEL_DOUBLES 16
#define PCR_LABEL_RESULT_DOUBLES 8
PCR_API int pcr_objects_match_labels(pcr_ctx* ctx, const pcr_objects* objs, const pcr_kitti_calib* calib, const double* labels /* L*16, host */, int64_t L,
                                     double* result /* L*8, host */, uint64_t* sel_bits /* L*words, host, or NULL */, int64_t words);

/* -------------------------------------------------------------- KITTI evaluation
 * What the reference runs on the label files it has written (Final_Project/README.md:225-236: `evaluate_object_3d_offline` of the
 * kitti_eval submodule, which the reference carries only as an empty directory): box overlaps, the greedy detection-to-label matching
 * and the average precision per class, metric and difficulty.  The tool's source is not part of the reference, so THIS COMMENT IS THE
 * DEFINITION; parity with the tool's own binary is UNPINNED.  tests/kitti_eval_checks.py restates the rules in NumPy.
 *
 * Rows.  A box is 16 doubles in the order of the label file (detection.KITTI_COLUMNS): 0 type, 1 truncated, 2 occluded, 3 alpha,
 *   4..7 left, top, right, bottom, 8..10 height, width, length, 11..13 cx, cy, cz, 14 ry, 15 score.  `type` is a code: 0 Car,
 *   1 Pedestrian, 2 Cyclist, 3 Van, 4 Person_sitting, 5 DontCare, 6 anything else.  Frames are ragged: frame f owns the detections
 *   det_first[f] .. det_first[f+1] and the labels gt_first[f] .. gt_first[f+1] (first[0] = 0, ascending).  A frame holds at most
 *   PCR_KITTI_EVAL_MAX_DET detections and PCR_KITTI_EVAL_MAX_GT labels: otherwise PCR_E_UNSUPPORTED, and nothing is written.
 *   Everything is binary64; cos(ry) and sin(ry) are taken on the host (no transcendental runs on the device).
 *
 * Overlap of a first box a (the detection) and a second box b, criterion c = -1 union, 0 the first box, 1 the second:
 *   ratio(i, A, B) = i / ((A + B) - i) for c = -1,  i / A for c = 0,  i / B for c = 1.
 *   image (metric 0):  w = min(right_a, right_b) - max(left_a, left_b),  h = min(bottom_a, bottom_b) - max(top_a, top_b), no +1;
 *     w <= 0 or h <= 0: 0;  otherwise ratio(w*h, (right_a-left_a)*(bottom_a-top_a), (right_b-left_b)*(bottom_b-top_b)).
 *   ground (metric 1): a box is the rectangle with local corners k = 0..3 (x, z) = (+l/2, +w/2), (-l/2, +w/2), (-l/2, -w/2),
 *     (+l/2, -w/2), mapped by X = (cos*x + sin*z) + ox, Z = (cos*z - sin*x) + oz; BOTH quads relative to the centre of a: for a
 *     (ox, oz) = (0, 0), for b (cx_b - cx_a, cz_b - cz_a) (absolute coordinates of some 50 m would cancel into areas of a few m^2).
 *     b's quad is clipped in turn by the lines through a's corners 0->1, 1->2, 2->3, 3->0.  With e = Q - P the side of a vertex is
 *     s = e_x*(Z - P_z) - e_z*(X - P_x), s >= 0 is inside (a vertex on the line is inside); the output takes, for every vertex V_i in
 *     order, V_i if inside and then, if V_i and its successor V_j differ in side, V_i + t*(V_j - V_i) with t = s_i/(s_i - s_j).
 *     area = 0.5 * sum over the vertices in order, from +0.0, of (X_i*Z_j - X_j*Z_i); fewer than 3 vertices or area <= 0: 0.
 *     ratio(area, l_a*w_a, l_b*w_b).  A box with l <= 0 or w <= 0 overlaps nothing.
 *   3-D (metric 2): hh = min(cy_a, cy_b) - max(cy_a - h_a, cy_b - h_b); hh <= 0 or a box with h <= 0: 0; otherwise
 *     ratio(area*hh, (h_a*l_a)*w_a, (h_b*l_b)*w_b).
 *   A field that is not finite among those a metric reads (image 4..7; ground 9, 10, 11, 13, 14; 3-D also 8, 12) makes it 0.
 *   pcr_kitti_box_overlap is this on the host for one pair (cos, sin from the C library); the kernel compiles the same source.
 *
 * Constants.  min_overlap[metric][class]: 0.7 / 0.5 / 0.5 for Car / Pedestrian / Cyclist in every metric by default (finite and
 *   >= 0, else PCR_E_INVALID).  Difficulty easy / moderate / hard: MIN_HEIGHT 40 / 25 / 25 on height2d = bottom - top,
 *   MAX_OCCLUSION 0 / 1 / 2, MAX_TRUNCATION 0.15 / 0.30 / 0.50.  PCR_KITTI_EVAL_SAMPLES = 41 recall sample points.
 *
 * Cleaning, per (class, difficulty).  A label of the class is IGNORED (flag 1) if occluded > MAX_OCCLUSION or truncated >
 *   MAX_TRUNCATION or height2d < MIN_HEIGHT, else COUNTED (flag 0; n_gt counts these).  A label of the neighbouring class (Van for
 *   Car, Person_sitting for Pedestrian) has flag 1.  DontCare rows form the frame's don't-care list.  Every other label is absent
 *   (flag -1).  A detection of the class has flag 1 if height2d < MIN_HEIGHT, else 0; other detections -1.
 *
 * Matching (the tool's computeStatistics), per frame, for a threshold t; mode 1 collects scores (t is not used), mode 2 counts.
 *   Labels in row order, skipping flag -1 and don't-care rows.  Per label, the detections in row order, skipping flag -1, assigned
 *   ones and, in mode 2, those with score < t; o = the metric's overlap (detection, label), c = -1; only o > min_overlap takes part.
 *     mode 1: the first such detection is the candidate; a later one replaces it only with a strictly greater score.
 *     mode 2: a flag-0 detection becomes the candidate if o > best (best starts at 0 and becomes o) or if the candidate has flag 1;
 *             a flag-1 detection becomes the candidate only while there is none (best stays).
 *   No candidate: fn += 1 if the label has flag 0.  A candidate is marked assigned; if neither it nor the label has flag 1,
 *   tp += 1, and mode 1 emits the candidate's score.
 *   Mode 2, after the labels: fp += 1 per detection that is unassigned, has flag 0 and score >= t.  Then for every don't-care row
 *   (outer loop, row order) and every such detection (inner loop): if the metric's overlap with c = 0 exceeds min_overlap, the
 *   detection is marked assigned and fp -= 1.  (KITTI's don't-care rows carry -1 / -1000 in their 3-D fields: they overlap nothing
 *   in the ground and 3-D metrics, by the rules above.)
 *
 * Thresholds and AP, per (class, metric, difficulty): v = the mode-1 scores of all frames, descending; current = 0; for i = 0 ..
 *   len-1: l = (i+1)/n_gt, r = (i+2)/n_gt if i < len-1 else l; if (r - current) < (current - l) and i < len-1, skip; otherwise
 *   emit v[i] and current += 1.0/40.0.  At most 41 are emitted.  For threshold k, with the mode-2 counts summed over the frames:
 *   recall[k] = tp/(double)(tp+fn), precision[k] = tp/(double)(tp+fp), 0 with a zero denominator; entries past n_thresholds are 0;
 *   then precision[k] = max(precision[k..40]).  ap11 = 100*(S/11.0), S = precision[0] + precision[4] + ... + precision[40] added in
 *   that order from +0.0; ap40 = 100*(S/40.0) over precision[1..40].  Orientation similarity is out of scope.
 *
 * The calls.  det / gt: host arrays of D x 16 and G x 16 doubles (NULL allowed when empty); det_first, gt_first: F + 1 entries.
 *   pcr_kitti_eval_overlaps: the three matrices for `criterion`, ragged: frame f's nd x ng block, detection-major, starts at
 *     pair_first[f]; any output may be NULL (each matrix holds pair_first[F] doubles, pair_first_out F + 1 entries).
 *   pcr_kitti_eval_match: one (cls, difficulty, metric) through the kernels of the whole evaluation.  mode 1: scores_out (capacity:
 *     the number of labels of the class) gets the emitted scores of all frames, descending, *n_scores_out their number, tp_out[0] /
 *     fn_out[0] the sums and fp_out[0] n_gt, the labels with flag 0 (one that takes a flag-1 detection is neither tp nor fn).  mode 2: tp_out, fp_out, fn_out [n_thresholds <= 41] for the given thresholds.  Outputs not named for a
 *     mode may be NULL and are left alone.
 *   pcr_kitti_eval: everything; result->cell[class][metric][difficulty].  stage_ms (3 doubles, or NULL): device time of the overlap
 *     pass, of mode 1 with the sort and the threshold pick, and of mode 2, by HIP events.  Thresholds are picked on the device; the
 *     only read-back is the final one.  The result depends on neither the order of the frames nor on the run.
 * PCR_E_INVALID: a NULL context, params or result; F < 0; first arrays NULL, not starting at 0 or descending; rows NULL while
 *   counted; cls, difficulty or metric outside 0..2; mode other than 1, 2; n_thresholds outside 0..41; criterion outside -1..1.    */
#define PCR_KITTI_EVAL_MAX_DET 256
#define PCR_KITTI_EVAL_MAX_GT 128
#define PCR_KITTI_EVAL_SAMPLES 41
#define PCR_KITTI_ROW_DOUBLES 16
typedef struct pcr_kitti_eval_params { double min_overlap[3][3]; /* [metric][class] */ double reserved[7]; } pcr_kitti_eval_params;
typedef struct pcr_kitti_eval_cell {
    int64_t n_gt, n_thresholds;
    double thresholds[PCR_KITTI_EVAL_SAMPLES];
    int64_t tp[PCR_KITTI_EVAL_SAMPLES], fp[PCR_KITTI_EVAL_SAMPLES], fn[PCR_KITTI_EVAL_SAMPLES];
    double precision[PCR_KITTI_EVAL_SAMPLES], recall[PCR_KITTI_EVAL_SAMPLES];
    double ap11, ap40;
} pcr_kitti_eval_cell;
typedef struct pcr_kitti_eval_result { pcr_kitti_eval_cell cell[3][3][3]; /* [class][metric][difficulty] */ } pcr_kitti_eval_result;
PCR_API void pcr_kitti_eval_default_params(pcr_kitti_eval_params* params);
PCR_API int pcr_kitti_box_overlap(const double a[16], const double b[16], int metric, int criterion, double* out);
PCR_API int pcr_kitti_eval_overlaps(pcr_ctx* ctx, const double* det, const int64_t* det_first, const double* gt, const int64_t* gt_first, int64_t F,
                                    int criterion, double* image_out, double* ground_out, double* volume_out, int64_t* pair_first_out);
PCR_API int pcr_kitti_eval_match(pcr_ctx* ctx, const double* det, const int64_t* det_first, const double* gt, const int64_t* gt_first, int64_t F,
                                 const pcr_kitti_eval_params* params, int cls, int difficulty, int metric, const double* thresholds, int n_thresholds,
                                 int mode, int64_t* tp_out, int64_t* fp_out, int64_t* fn_out, double* scores_out, int64_t* n_scores_out);
PCR_API int pcr_kitti_eval(pcr_ctx* ctx, const double* det, const int64_t* det_first, const double* gt, const int64_t* gt_first, int64_t F,
                           const pcr_kitti_eval_params* params, pcr_kitti_eval_result* result, double* stage_ms);

/* ------------------------------------------------------------- timing aid
 * HIP-event stopwatch on the ctx stream, for bench.py's roofline figures.   */
PCR_API int pcr_timer_start(pcr_ctx* ctx);
PCR_API int pcr_timer_stop_ms(pcr_ctx* ctx, double* ms_out);
/* Per-kernel HIP-event profile of the ICP pass (adds one event sync per pass while on).
 * slots: 0 = the one-launch ICP pass (grid: tiles, work queue, moments, Procrustes step; in the two-launch variant and in
 *        ungated runs: the tile launch) / MFMA sweep (brute), 1 = the drain launch of the two-launch variant (ungated runs:
 *        hard stage) / merge + exact fallback (brute), 2 = separate accumulate kernel (grid, ungated runs only) / final
 *        (brute), 3 = reduce (brute).
 * ms_out[4] = summed milliseconds (each slot includes the launch gap in front of it), *passes_out = passes profiled. */
/* diagnostics: per-block {cycles, work} stamps of the last grid search stage kernels (PCR_DEBUG_STAMPS=1) */
PCR_API int pcr_debug_read(pcr_ctx* ctx, uint64_t* out, int64_t n_words);
/* diagnostics of the context's device arena: out[0] = blocks handed out and not yet given back, out[1] = their bytes.  Equal before
 * and after a call that returned no handle, whatever its status.                                                                  */
PCR_API int pcr_debug_arena(pcr_ctx* ctx, int64_t out[2]);
/* diagnostics: the nth next device-scratch allocation on this context is refused (PCR_E_NOMEM), once; nth = 0 disarms.  Only a counter
 * on the host is tested: nothing is launched and no device call is made to fail.  Not for the batch entry points.             */
PCR_API int pcr_debug_fail_alloc(pcr_ctx* ctx, int nth);
/* diagnostics: n independent problems through one of the small dense solves that end the hot paths (csrc/pcr_linalg.h), one problem
 * per device lane, so that tests reach the DEVICE build of each function with inputs no pipeline produces.  ctx == NULL: the same loop
 * through the host build.  Doubles per problem, row-major matrices:
 *   op 0  svd3                      in H[9]                          out U[9], s[3], V[9]
 *   op 1  svd3, warm start          in H[9], V0[9]                   out U[9], s[3], V[9]
 *   op 2  sym3_jacobi               in upper triangle 00 01 02 11 12 22   out A after [9], Q[9]
 *   op 3  kabsch_from_moments       in m[18], origin[3]              out R[9], t[3], cost
 *   op 4  the same with V_io        in m[18], origin[3], V[9]        out R[9], t[3], cost, V[9]
 *   op 5  point2plane_solve         in A_upper[21], b[6]             out x[6], U[16], ok (1.0 / 0.0)
 * n == 0: PCR_OK, nothing written.  PCR_E_INVALID: n < 0, n > 65536, an unknown op, in or out NULL.                                */
PCR_API int pcr_debug_linalg(pcr_ctx* ctx, int op, const double* in, int64_t n, double* out);
PCR_API int pcr_profile_enable(pcr_ctx* ctx, int on);
/* diagnostics of the LAST correspondence search on this context (Registration/main.py:116-121 is the step they describe):
 * out[0] = queries the brute-force MFMA sweep could not prove and re-did with the exact direct-form sweep;
 * out[1] = device arenas (256-MiB hipMalloc blocks the context's buffers are carved from) allocated since the context was
 * created, out[2] = microseconds of host time those allocations took, out[3] = arenas held now: a call that had to grow an
 * arena pays milliseconds on the host with its stream idle, and a caller timing calls can name that.
 * Exactness never depends on these numbers; tests use out[0] to see the fallback fire.   */
PCR_API int pcr_search_stats(pcr_ctx* ctx, int64_t out[4]);

/* Per-pass log of the LAST pcr_icp call on this context that ran the device-resident loop (grid index, gated): for every association
 * pass (Registration/main.py:107-154 is one) the duration of its tile launch -- of the whole pass when it ran as one launch --, of
 * its drain launch (0 for a one-launch pass) and the queries the tiles handed to the work queue (two-launch passes), from the
 * kernels' own 100-MHz timestamps.  *n_out = passes logged (<= PCR_ICP_MAX_LOG); at most max_n entries are written.
 * host_us (may be NULL): the call on the host, microseconds -- [0] set-up before the first launch, [1] enqueueing the first chunk
 * of passes, [2] waiting for the device (all synchronisations), [3] the whole loop, [4] by HIP events: from the start of the call to
 * behind the last kernel of the last chunk (in front of the read-back of the loop state), [5] the last wait alone.                 */
PCR_API int pcr_icp_pass_log(pcr_ctx* ctx, int max_n, double* tile_us, double* drain_us, int64_t* items, int* n_out, double host_us[6]);

/* Scheduling hint: shared != 0 tells the library that other contexts keep the same device busy while this one runs ICP
 * loops (a batch worker: Registration/main.py:190-216 spread over several streams).  The ICP pass then runs as two launches
 * instead of one whose idle waves wait in place for work -- latency for one pair bought with wave slots the other pairs
 * could use.  Results are identical bit for bit either way.  pcr_icp_batch sets it for its own worker contexts; without
 * the hint the library still switches by itself while it sees more than one loop of the process in flight. */
PCR_API int pcr_ctx_set_shared(pcr_ctx* ctx, int shared);
PCR_API int pcr_profile_read(pcr_ctx* ctx, double ms_out[4], int* passes_out);

#ifdef __cplusplus
}
#endif
#endif /* PCR_H */
