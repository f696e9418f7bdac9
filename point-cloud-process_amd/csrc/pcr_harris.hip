// Harris-3D and PCL-rule ISS keypoints -- the XYZ detectors of PCLKeypoints/src/keypoints.cpp (keypointHarris3D, keypointIss), by the
// rules stated in include/pcr.h (PCL itself is not part of the build: parity with its binary32 output is unpinned).
// All passes walk the radius neighbourhood by pcr_ball_visit.h (the lane-group walk, 8 lanes per point; the note at the top of
// pcr_iss.hip says why per-point lanes and not wave tiles; refine: the wave walk), in binary64, and every sum
// runs in a fixed order -- a lane's cells in lane order, a cell's records in stored order, then the lanes -- so a call is repeatable
// to the bit.  Per-row results are stored BY CALLER ROW (the record's id): a cloud that an index has laid out along its curve takes
// and returns caller rows like any other.
//   position covariance   sum x, sum x x^T over x = p_j - p_i  ->  the radius normal (smallest eigenvector, pcr::sym3_jacobi) and |N|,
//                         or (SCATTER) the PCL-rule ISS score from the unweighted scatter's eigenvalues
//   normal covariance     sum n_j n_j^T over the neighbours with a finite normal (24 B gathered per neighbour, by row)  ->  response
//   suppression           one flag per row: a candidate that no row of its ball beats; rocprim::select over the row numbers follows,
//                         so the keypoints come out in ascending caller row and only they (and their count) cross PCIe
//   refine                one wave per corner, the 64 lanes stride through the 27 cells' records: up to 5 rounds of c <- (sum n n^T)^-1 sum (n n^T) p
// Nothing adds with atomics, and the host reads nothing back between the passes (the count of selected rows is the first read).
#include <cmath>
#include <cstring>
#include <string>
#include "pcr_ball_visit.h"
#include "pcr_linalg.h"
#include "pcr_sort.h"

template <bool SCATTER>
__global__ void __launch_bounds__(256) harris_poscov_kernel(pcr_grid_view gv, long long n, double r2_in, double vx, double vy, double vz, double gamma21,
                                                            double gamma32, double* __restrict__ out /* by row: normals (n,3) | SCATTER: score (n) */,
                                                            int* __restrict__ counts /* by row, or null */) {
    long long i;
    int gl;
    if (!ball_lane_point(n, &i, &gl)) return;
    const pcr_pt p = gv.pts[i];
    double m[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // x y z, xx xy xz yy yz zz
    int c = 0;
    auto f = [&](const pcr_pt& b, unsigned int) {
        const double dx = b.x - p.x, dy = b.y - p.y, dz = b.z - p.z;
        if ((dx * dx + dy * dy) + dz * dz <= r2_in) {
            ++c;
            if (!SCATTER) { m[0] += dx; m[1] += dy; m[2] += dz; }
            m[3] += dx * dx; m[4] += dx * dy; m[5] += dx * dz;
            m[6] += dy * dy; m[7] += dy * dz; m[8] += dz * dz;
        }
    };
    ball_visit<BALL_LANES>(gv, p.x, p.y, p.z, gl, f);
#pragma unroll
    for (int k = SCATTER ? 3 : 0; k < 9; ++k) m[k] = ball_lanes_sum(m[k]);
    c = ball_lanes_sum(c);
    if (gl != 0) return;
    if (counts) counts[p.id] = c;
    double Q[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    if (SCATTER) {
        double A[3][3] = {{m[3], m[4], m[5]}, {m[4], m[6], m[7]}, {m[5], m[7], m[8]}};
        pcr::sym3_jacobi(A, Q);
        double e1 = A[0][0], e2 = A[1][1], e3 = A[2][2];
        if (e1 < e2) { const double t = e1; e1 = e2; e2 = t; }
        if (e2 < e3) { const double t = e2; e2 = e3; e3 = t; }
        if (e1 < e2) { const double t = e1; e1 = e2; e2 = t; }
        const bool ok = e1 > 0.0 && e2 > 0.0 && e3 >= 0.0 && e2 / e1 < gamma21 && e3 / e2 < gamma32;
        out[p.id] = ok ? e3 : 0.0;
        return;
    }
    double nx = NAN, ny = NAN, nz = NAN;
    if (c >= 3) {
        const double cd = (double)c, mx = m[0] / cd, my = m[1] / cd, mz = m[2] / cd;
        double A[3][3];
        A[0][0] = m[3] / cd - mx * mx; A[0][1] = A[1][0] = m[4] / cd - mx * my; A[0][2] = A[2][0] = m[5] / cd - mx * mz;
        A[1][1] = m[6] / cd - my * my; A[1][2] = A[2][1] = m[7] / cd - my * mz; A[2][2] = m[8] / cd - mz * mz;
        pcr::sym3_jacobi(A, Q);
        // the column of the smallest eigenvalue, by selects (a run-time column index would put Q into scratch memory)
        const double d0 = A[0][0], d1 = A[1][1], d2 = A[2][2];
        const bool k0 = d0 <= d1 && d0 <= d2, k1 = !k0 && d1 <= d2;
        nx = k0 ? Q[0][0] : (k1 ? Q[0][1] : Q[0][2]);
        ny = k0 ? Q[1][0] : (k1 ? Q[1][1] : Q[1][2]);
        nz = k0 ? Q[2][0] : (k1 ? Q[2][1] : Q[2][2]);
        const double len = sqrt((nx * nx + ny * ny) + nz * nz);
        nx /= len; ny /= len; nz /= len;
        if ((nx * (vx - p.x) + ny * (vy - p.y)) + nz * (vz - p.z) < 0.0) { nx = -nx; ny = -ny; nz = -nz; }
    }
    out[3 * p.id + 0] = nx;
    out[3 * p.id + 1] = ny;
    out[3 * p.id + 2] = nz;
}

__global__ void __launch_bounds__(256) harris_response_kernel(pcr_grid_view gv, long long n, double r2_in, const double* __restrict__ nrm /* by row (n,3) */,
                                                              double* __restrict__ resp /* by row */, int* __restrict__ counts /* by row, or null */) {
    long long i;
    int gl;
    if (!ball_lane_point(n, &i, &gl)) return;
    const pcr_pt p = gv.pts[i];
    double m[6] = {0, 0, 0, 0, 0, 0};   // xx xy xz yy yz zz of the normals
    int k = 0, c = 0;
    auto f = [&](const pcr_pt& b, unsigned int) {
        if (dist2(p.x, p.y, p.z, b) <= r2_in) {
            ++c;
            const double* q = nrm + 3 * b.id;
            const double a0 = q[0], a1 = q[1], a2 = q[2];
            if (finite3(a0, a1, a2)) {
                ++k;
                m[0] += a0 * a0; m[1] += a0 * a1; m[2] += a0 * a2;
                m[3] += a1 * a1; m[4] += a1 * a2; m[5] += a2 * a2;
            }
        }
    };
    ball_visit<BALL_LANES>(gv, p.x, p.y, p.z, gl, f);
#pragma unroll
    for (int j = 0; j < 6; ++j) m[j] = ball_lanes_sum(m[j]);
    k = ball_lanes_sum(k);
    c = ball_lanes_sum(c);
    if (gl != 0) return;
    if (counts) counts[p.id] = c;
    const double* own = nrm + 3 * p.id;
    double r = 0.0;
    if (k > 0 && finite3(own[0], own[1], own[2])) {
        const double kd = (double)k;
        const double xx = m[0] / kd, xy = m[1] / kd, xz = m[2] / kd, yy = m[3] / kd, yz = m[4] / kd, zz = m[5] / kd;
        const double trace = xx + yy + zz;
        if (trace != 0.0) {
            const double det = xx * yy * zz + 2.0 * xy * xz * yz - xz * xz * yy - xy * xy * zz - yz * yz * xx;
            r = 0.04 + det - 0.04 * trace * trace;
        }
    }
    resp[p.id] = r;
}

// flags[row] = 1: the row is a candidate (score >= thr, or > thr when strict; at least min_nb rows in its ball) and no row of its ball has
// a strictly greater score.  Rows that fail the score test skip the walk unless their count is asked for.
__global__ void __launch_bounds__(256) harris_suppress_kernel(pcr_grid_view gv, long long n, double r2_in, const double* __restrict__ score /* by row */, double thr,
                                                              int strict, int min_nb, unsigned char* __restrict__ flags /* by row */,
                                                              int* __restrict__ counts /* by row, or null */, unsigned int* __restrict__ row_pos /* by row, or null */) {
    long long i;
    int gl;
    if (!ball_lane_point(n, &i, &gl)) return;
    const pcr_pt p = gv.pts[i];
    const double s = score[p.id];
    const bool cand = strict ? s > thr : s >= thr;
    if (gl == 0 && row_pos) row_pos[p.id] = (unsigned int)i;
    if (!cand && !counts) {   // (the 8 lanes of a point leave together)
        if (gl == 0) flags[p.id] = 0;
        return;
    }
    int c = 0, beaten = 0;
    auto f = [&](const pcr_pt& b, unsigned int) {
        if (dist2(p.x, p.y, p.z, b) <= r2_in) {
            ++c;
            beaten += score[b.id] > s;
        }
    };
    ball_visit<BALL_LANES>(gv, p.x, p.y, p.z, gl, f);
    c = ball_lanes_sum(c);
    beaten = ball_lanes_sum(beaten);
    if (gl != 0) return;
    if (counts) counts[p.id] = c;
    flags[p.id] = (cand && c >= min_nb && beaten == 0) ? 1 : 0;
}

__global__ void harris_gather_kernel(const double* __restrict__ score, const int* __restrict__ rows, unsigned int m, double* __restrict__ out) {
    const unsigned int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < m) out[j] = score[rows[j]];
}

// One wave per corner.  The corner moves: it is no cloud row after the first round and may leave the grid -- cells outside the
// representable range or absent from the table are empty, and a corner that is not finite meets no record at all.
__global__ void __launch_bounds__(64) harris_refine_kernel(pcr_grid_view gv, const int* __restrict__ rows, const unsigned int* __restrict__ row_pos, double r2_in,
                                                           const double* __restrict__ nrm /* by row */, double* __restrict__ refined /* (k,3) */,
                                                           int* __restrict__ rounds /* k */) {
    const int lane = threadIdx.x;
    const pcr_pt p0 = gv.pts[row_pos[rows[blockIdx.x]]];
    double cx = p0.x, cy = p0.y, cz = p0.z;
    int round = 0;
    while (round < 5) {
        double m[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // A: xx xy xz yy yz zz, b: x y z
        // the wave walk of pcr_ball_visit.h: a lane's terms come in a fixed order
        auto f = [&](unsigned int j, bool valid) {
            if (!valid) return;
            const pcr_pt b = gv.pts[j];
            if (dist2(cx, cy, cz, b) <= r2_in) {
                const double* q = nrm + 3 * b.id;
                const double a0 = q[0], a1 = q[1], a2 = q[2];
                if (finite3(a0, a1, a2)) {
                    const double xx = a0 * a0, xy = a0 * a1, xz = a0 * a2, yy = a1 * a1, yz = a1 * a2, zz = a2 * a2;
                    m[0] += xx; m[1] += xy; m[2] += xz; m[3] += yy; m[4] += yz; m[5] += zz;
                    m[6] += (xx * b.x + xy * b.y) + xz * b.z;
                    m[7] += (xy * b.x + yy * b.y) + yz * b.z;
                    m[8] += (xz * b.x + yz * b.y) + zz * b.z;
                }
            }
        };
        unsigned int s, e;
        wave_block_runs(gv, cx, cy, cz, lane, &s, &e);
        wave_visit_runs(s, e, lane, f);
#pragma unroll
        for (int k = 0; k < 9; ++k) m[k] = wave_sum_all(m[k]);   // the 64 lanes in a fixed order; every lane ends with the same bits
        ++round;
        const double xx = m[0], xy = m[1], xz = m[2], yy = m[3], yz = m[4], zz = m[5];
        const double det = xx * yy * zz + 2.0 * xy * xz * yz - xz * xz * yy - xy * xy * zz - yz * yz * xx;
        double qx = cx, qy = cy, qz = cz;
        if (det != 0.0) {   // c <- A^-1 b by the adjugate
            const double i00 = yy * zz - yz * yz, i01 = xz * yz - xy * zz, i02 = xy * yz - xz * yy;
            const double i11 = xx * zz - xz * xz, i12 = xy * xz - xx * yz, i22 = xx * yy - xy * xy;
            qx = ((i00 * m[6] + i01 * m[7]) + i02 * m[8]) / det;
            qy = ((i01 * m[6] + i11 * m[7]) + i12 * m[8]) / det;
            qz = ((i02 * m[6] + i12 * m[7]) + i22 * m[8]) / det;
        }
        const double dx = qx - cx, dy = qy - cy, dz = qz - cz;
        const double move2 = (dx * dx + dy * dy) + dz * dz;
        cx = qx; cy = qy; cz = qz;
        if (!(move2 > 1e-6)) break;
    }
    if (lane == 0) {
        refined[3 * blockIdx.x + 0] = cx;
        refined[3 * blockIdx.x + 1] = cy;
        refined[3 * blockIdx.x + 2] = cz;
        if (rounds) rounds[blockIdx.x] = round;
    }
}

// the flagged rows in ascending row -> b_rows (device, n ints), their number -> *n_sel and *n_keypoints_out, the rows themselves -> keypoints_out;
// a buffer that cannot hold them: the needed count and PCR_E_UNSUPPORTED
static int harris_select(pcr_ctx* ctx, int64_t n, const unsigned char* d_flags, const char* who, pcr_dev_block& b_rows, int32_t* keypoints_out, int64_t capacity,
                         int64_t* n_keypoints_out, unsigned int* n_sel) {
    pcr_dev_block b_cnt(ctx), b_tmp(ctx);
    int rc;
    if ((rc = b_rows.alloc(sizeof(int) * n)) || (rc = b_cnt.alloc(sizeof(unsigned int)))) return rc;
    if ((rc = pcr_select_positions(ctx, d_flags, (size_t)n, b_rows.as<int>(), b_cnt.as<unsigned int>(), b_tmp, who))) return rc;
    if ((rc = pcr_d2h_small(ctx, n_sel, b_cnt.p, sizeof(unsigned int)))) return rc;
    *n_keypoints_out = (int64_t)*n_sel;
    if ((int64_t)*n_sel > capacity) {
        ctx->last_error = std::string(who) + ": the keypoint buffer holds " + std::to_string(capacity) + " rows, " + std::to_string(*n_sel) + " are needed";
        return PCR_E_UNSUPPORTED;
    }
    return pcr_d2h_small(ctx, keypoints_out, b_rows.p, sizeof(int) * (size_t)*n_sel);
}

extern "C" void pcr_harris_default_params(pcr_harris_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->radius = 0.5;        // keypoints.cpp:253-257
    p->threshold = 0.001;
}

extern "C" int pcr_normals_radius(pcr_ctx* ctx, const pcr_cloud* cloud, double radius, const double* viewpoint, double* normals_out, int32_t* counts_out) try {
    if (!ctx || !cloud || !normals_out || !(radius > 0) || !std::isfinite(radius)) return PCR_E_INVALID;
    if (viewpoint && !(std::isfinite(viewpoint[0]) && std::isfinite(viewpoint[1]) && std::isfinite(viewpoint[2]))) return PCR_E_INVALID;
    if (cloud->n <= 0) return PCR_E_EMPTY;
    hipSetDevice(ctx->device);
    const int64_t n = cloud->n;
    pcr_index_guard idx(ctx);
    int rc = ball_grid(ctx, cloud, radius, "pcr_normals_radius", idx);
    if (rc) return rc;
    pcr_dev_block b_nrm(ctx), b_counts(ctx);
    if ((rc = b_nrm.alloc(sizeof(double) * 3 * n)) || (counts_out && (rc = b_counts.alloc(sizeof(int) * n)))) return rc;
    const double vx = viewpoint ? viewpoint[0] : 0.0, vy = viewpoint ? viewpoint[1] : 0.0, vz = viewpoint ? viewpoint[2] : 0.0;
    hipLaunchKernelGGL(harris_poscov_kernel<false>, dim3(ball_blocks(n)), dim3(256), 0, ctx->stream, idx->view, (long long)n, radius * radius, vx, vy, vz, 0.0, 0.0,
                       b_nrm.as<double>(), b_counts.as<int>());
    PCR_HIP(ctx, hipGetLastError());
    if ((rc = pcr_d2h_staged(ctx, normals_out, b_nrm.p, sizeof(double) * 3 * (size_t)n))) return rc;
    if (counts_out && (rc = pcr_d2h_staged(ctx, counts_out, b_counts.p, sizeof(int) * (size_t)n))) return rc;
    return PCR_OK;
} PCR_CATCH(ctx)

extern "C" int pcr_harris3d(pcr_ctx* ctx, const pcr_cloud* cloud, const double* normals, const pcr_harris_params* params, double* response_out, int32_t* counts_out,
                            int32_t* keypoints_out, int64_t capacity, int64_t* n_keypoints_out, double* keypoint_response_out, double* refined_out,
                            int32_t* rounds_out) try {
    if (!ctx || !cloud || !params) return PCR_E_INVALID;
    const double radius = params->radius, thr = params->threshold;
    if (!(radius > 0) || !std::isfinite(radius) || !std::isfinite(thr)) return PCR_E_INVALID;
    const bool want_kp = keypoints_out != nullptr;
    if (want_kp && (!n_keypoints_out || capacity < 0)) return PCR_E_INVALID;
    if (!want_kp && (keypoint_response_out || refined_out || rounds_out)) return PCR_E_INVALID;   // per-keypoint results without the keypoints
    if (!want_kp && !response_out && !counts_out) return PCR_E_INVALID;                             // nothing asked for
    if (cloud->n <= 0) return PCR_E_EMPTY;
    hipSetDevice(ctx->device);
    const int64_t n = cloud->n;
    const bool nms = params->nms != 0, refine = nms && params->refine != 0 && refined_out;
    pcr_index_guard idx(ctx);
    int rc = ball_grid(ctx, cloud, radius, "pcr_harris3d", idx);
    if (rc) return rc;
    pcr_dev_block b_nrm(ctx), b_resp(ctx), b_counts(ctx);
    if ((rc = b_nrm.alloc(sizeof(double) * 3 * n)) || (rc = b_resp.alloc(sizeof(double) * n)) || (counts_out && (rc = b_counts.alloc(sizeof(int) * n)))) return rc;
    const double r2_in = radius * radius;
    const unsigned grid = ball_blocks(n);
    if (normals) PCR_HIP(ctx, hipMemcpyAsync(b_nrm.p, normals, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    else hipLaunchKernelGGL(harris_poscov_kernel<false>, dim3(grid), dim3(256), 0, ctx->stream, idx->view, (long long)n, r2_in, 0.0, 0.0, 0.0, 0.0, 0.0, b_nrm.as<double>(),
                            (int*)nullptr);
    hipLaunchKernelGGL(harris_response_kernel, dim3(grid), dim3(256), 0, ctx->stream, idx->view, (long long)n, r2_in, (const double*)b_nrm.p, b_resp.as<double>(),
                       b_counts.as<int>());
    PCR_HIP(ctx, hipGetLastError());
    if (!want_kp || !nms) {
        // every row with its response: nothing to select (the stream is synchronised before the caller's normals may change)
        if (response_out && (rc = pcr_d2h_staged(ctx, response_out, b_resp.p, sizeof(double) * (size_t)n))) return rc;
        if (counts_out && (rc = pcr_d2h_staged(ctx, counts_out, b_counts.p, sizeof(int) * (size_t)n))) return rc;
        if (!response_out && !counts_out) PCR_HIP(ctx, pcr_sync(ctx->stream));
        if (want_kp) {
            *n_keypoints_out = n;
            if (n > capacity) {
                ctx->last_error = "pcr_harris3d: the keypoint buffer holds " + std::to_string(capacity) + " rows, " + std::to_string(n) + " are needed";
                return PCR_E_UNSUPPORTED;
            }
            for (int64_t i = 0; i < n; ++i) keypoints_out[i] = (int32_t)i;
            if (keypoint_response_out) {
                if (response_out) memcpy(keypoint_response_out, response_out, sizeof(double) * (size_t)n);
                else if ((rc = pcr_d2h_staged(ctx, keypoint_response_out, b_resp.p, sizeof(double) * (size_t)n))) return rc;
            }
        }
        return PCR_OK;
    }
    pcr_dev_block b_flags(ctx), b_pos(ctx), b_rows(ctx);
    if ((rc = b_flags.alloc((size_t)n)) || (refine && (rc = b_pos.alloc(sizeof(unsigned int) * n)))) return rc;
    hipLaunchKernelGGL(harris_suppress_kernel, dim3(grid), dim3(256), 0, ctx->stream, idx->view, (long long)n, r2_in, (const double*)b_resp.p, thr, 0, 0,
                       b_flags.as<unsigned char>(), (int*)nullptr, b_pos.as<unsigned int>());
    PCR_HIP(ctx, hipGetLastError());
    unsigned int k = 0;
    rc = harris_select(ctx, n, b_flags.as<unsigned char>(), "pcr_harris3d", b_rows, keypoints_out, capacity, n_keypoints_out, &k);
    // (the per-row results are the caller's even when the keypoint buffer was too small)
    int rc2;
    if (response_out && (rc2 = pcr_d2h_staged(ctx, response_out, b_resp.p, sizeof(double) * (size_t)n))) return rc2;
    if (counts_out && (rc2 = pcr_d2h_staged(ctx, counts_out, b_counts.p, sizeof(int) * (size_t)n))) return rc2;
    if (rc || k == 0) return rc;
    if (keypoint_response_out) {
        pcr_dev_block b_ks(ctx);
        if ((rc = b_ks.alloc(sizeof(double) * k))) return rc;
        hipLaunchKernelGGL(harris_gather_kernel, dim3((k + 255) / 256), dim3(256), 0, ctx->stream, (const double*)b_resp.p, (const int*)b_rows.p, k, b_ks.as<double>());
        PCR_HIP(ctx, hipGetLastError());
        if ((rc = pcr_d2h_small(ctx, keypoint_response_out, b_ks.p, sizeof(double) * k))) return rc;
    }
    if (refine) {
        pcr_dev_block b_ref(ctx), b_rounds(ctx);
        if ((rc = b_ref.alloc(sizeof(double) * 3 * k)) || (rc = b_rounds.alloc(sizeof(int) * k))) return rc;
        hipLaunchKernelGGL(harris_refine_kernel, dim3(k), dim3(64), 0, ctx->stream, idx->view, (const int*)b_rows.p, (const unsigned int*)b_pos.p, r2_in,
                           (const double*)b_nrm.p, b_ref.as<double>(), b_rounds.as<int>());
        PCR_HIP(ctx, hipGetLastError());
        if ((rc = pcr_d2h_small(ctx, refined_out, b_ref.p, sizeof(double) * 3 * k))) return rc;
        if (rounds_out && (rc = pcr_d2h_small(ctx, rounds_out, b_rounds.p, sizeof(int) * k))) return rc;
    }
    return PCR_OK;
} PCR_CATCH(ctx)

extern "C" int pcr_iss_pcl(pcr_ctx* ctx, const pcr_cloud* cloud, double salient_radius, double non_max_radius, double gamma21, double gamma32, int min_neighbors,
                           double* e3_out, int32_t* counts_out, int32_t* keypoints_out, int64_t capacity, int64_t* n_keypoints_out) try {
    if (!ctx || !cloud) return PCR_E_INVALID;
    if (!(salient_radius > 0) || !std::isfinite(salient_radius) || !(non_max_radius > 0) || !std::isfinite(non_max_radius)) return PCR_E_INVALID;
    if (std::isnan(gamma21) || std::isnan(gamma32)) return PCR_E_INVALID;
    const bool want_kp = keypoints_out != nullptr;
    if (want_kp && (!n_keypoints_out || capacity < 0)) return PCR_E_INVALID;
    if (!want_kp && !e3_out && !counts_out) return PCR_E_INVALID;   // nothing asked for
    if (cloud->n <= 0) return PCR_E_EMPTY;
    hipSetDevice(ctx->device);
    const int64_t n = cloud->n;
    // one grid serves both radii: the 3x3x3 block of a cell of the larger radius covers either ball
    pcr_index_guard idx(ctx);
    int rc = ball_grid(ctx, cloud, salient_radius > non_max_radius ? salient_radius : non_max_radius, "pcr_iss_pcl", idx);
    if (rc) return rc;
    pcr_dev_block b_score(ctx), b_counts(ctx), b_flags(ctx), b_rows(ctx);
    if ((rc = b_score.alloc(sizeof(double) * n)) || (counts_out && (rc = b_counts.alloc(sizeof(int) * n))) || (rc = b_flags.alloc((size_t)n))) return rc;
    const unsigned grid = ball_blocks(n);
    hipLaunchKernelGGL(harris_poscov_kernel<true>, dim3(grid), dim3(256), 0, ctx->stream, idx->view, (long long)n, salient_radius * salient_radius, 0.0, 0.0, 0.0, gamma21,
                       gamma32, b_score.as<double>(), (int*)nullptr);
    if (want_kp || counts_out)
        hipLaunchKernelGGL(harris_suppress_kernel, dim3(grid), dim3(256), 0, ctx->stream, idx->view, (long long)n, non_max_radius * non_max_radius,
                           (const double*)b_score.p, 0.0, 1, min_neighbors, b_flags.as<unsigned char>(), b_counts.as<int>(), (unsigned int*)nullptr);
    PCR_HIP(ctx, hipGetLastError());
    unsigned int k = 0;
    rc = PCR_OK;
    if (want_kp) rc = harris_select(ctx, n, b_flags.as<unsigned char>(), "pcr_iss_pcl", b_rows, keypoints_out, capacity, n_keypoints_out, &k);
    int rc2;
    if (e3_out && (rc2 = pcr_d2h_staged(ctx, e3_out, b_score.p, sizeof(double) * (size_t)n))) return rc2;
    if (counts_out && (rc2 = pcr_d2h_staged(ctx, counts_out, b_counts.p, sizeof(int) * (size_t)n))) return rc2;
    return rc;
} PCR_CATCH(ctx)
