// Object batches: the stage between DBSCAN's labels and the classifier's input, `preprocess` of Final_Project/scripts/detect.py:269-354
// (and the resampling of generating-training-set.py:186-194), on a device-resident cloud.
//
// pcr_objects_build groups the labelled rows by object id, ascending caller row within an object (the record's id: the device copy of a
// cloud may have been re-laid along an index's curve), and leaves per-object statistics beside them.  The labels arrive on the host, so
// the argument check and the per-object counts are one pass over them there; everything that touches a point runs on the device:
//   objects_keys_kernel      key = the row's object id (noise: n_objects, sorted behind every object), value = the row;
//   pcr_sort_pairs           rocPRIM's radix sort, stable: equal ids keep their ascending rows;
//   objects_dst_kernel       where every labelled row goes in the grouped order (-1: noise);
//   objects_scatter_kernel   every record of the cloud looks its id up there;
//   objects_stats_kernel     one wave per object: coordinate sums in ascending row order (np.mean's order, detect.py:290,312), min, max.
// pcr_objects_weights is the hot path, squareform(pdist(P_o)).mean(axis=0) of detect.py:299-301 without the n x n matrix:
//   objects_tiles_kernel     the work list of (object, block of 64 i rows) tiles from the offsets and the keep flags, objects with more
//                            rows in front (by power of two of their count: the order only decides which tile starts first);
//   objects_weights_kernel   one wave per tile, lane i owns row i's running sum; the object's rows go by in ascending order, staged
//                            through LDS PCR_OBJECTS_TILE at a time and read back as broadcasts.
// pcr_objects_pack_f32 writes the classifier's float32 batch (detect.py:311-318) into the caller's device tensor.
// pcr_objects_kitti_boxes is the detector's back end, the per-object part of to_kitti_eval_format (detect.py:106-163):
//   kitti_boxes_kernel       one wave per object, three passes over its rows: camera frame + pixel box + coordinate sums, the centred
//                            x-z moments and the heading direction (kitti_direction_rule, shared with the host's
//                            pcr_kitti_direction), the extents in the heading-aligned frame.  An object of at most PCR_KITTI_LDS_ROWS
//                            rows keeps its camera-frame rows in LDS between the passes; a larger one computes them again.
// Every floating-point result is a fixed sequence of binary64 operations without contraction: nothing depends on arrival order.
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>
#include "pcr_internal.h"
#include "pcr_kitti_dev.h"
#include "pcr_sort.h"
#include "pcr_wave.h"

namespace {

constexpr int OB_WAVE = 64;                  // i rows per tile = lanes of the one wave that owns it
constexpr int OB_J = PCR_OBJECTS_TILE;       // j rows per LDS stage
constexpr int OB_BLOCK = 256;
static_assert(OB_J % OB_WAVE == 0, "a stage is loaded by whole waves");

struct ob_tile { int object, iblock; };

__global__ void __launch_bounds__(OB_BLOCK)
objects_keys_kernel(const int* __restrict__ labels, long long n, unsigned int noise_key, unsigned int* __restrict__ keys, unsigned int* __restrict__ vals) {
    const long long row = (long long)blockIdx.x * OB_BLOCK + threadIdx.x;
    if (row >= n) return;
    const int l = labels[row];
    keys[row] = l < 0 ? noise_key : (unsigned int)l;
    vals[row] = (unsigned int)row;
}

// dst[row] = place of a labelled row in the grouped order (the first m sorted pairs are the labelled ones); dst is -1 elsewhere
__global__ void __launch_bounds__(OB_BLOCK)
objects_dst_kernel(const unsigned int* __restrict__ rows_sorted, long long m, int* __restrict__ dst) {
    const long long k = (long long)blockIdx.x * OB_BLOCK + threadIdx.x;
    if (k < m) dst[rows_sorted[k]] = (int)k;
}

__global__ void __launch_bounds__(OB_BLOCK)
objects_scatter_kernel(const pcr_pt* __restrict__ pts, long long n, const int* __restrict__ dst, long long m, pcr_pt* __restrict__ recs) {
    const long long i = (long long)blockIdx.x * OB_BLOCK + threadIdx.x;
    if (i >= n) return;
    const pcr_pt p = pts[i];
    if (p.id < 0 || p.id >= n) return;   // (the ids of a cloud are a permutation of [0, n))
    const int d = dst[p.id];
    if (d >= 0 && d < m) recs[d] = p;
}

// One wave per object.  64 records at a time go through LDS; lanes 0..2 add one axis each in ascending row order -- a dependent add
// chain as long as the object, which is what bounds this step -- while every lane keeps the min / max of the records it loaded.
// An object of count 0: 0.0 / 0.0 = NaN, min +inf, max -inf.
__global__ void __launch_bounds__(OB_WAVE)
objects_stats_kernel(const pcr_pt* __restrict__ recs, const long long* __restrict__ off, double* __restrict__ stats) {
    __shared__ double s_c[3][OB_WAVE];
    const int lane = threadIdx.x;
    const long long o = blockIdx.x;
    const long long base = off[o];
    const int cnt = (int)(off[o + 1] - base);
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    double mn[3] = {inf, inf, inf}, ng[3] = {inf, inf, inf};   // ng: minimum of the negated coordinate
    double sum = 0.0;
    for (int j0 = 0; j0 < cnt; j0 += OB_WAVE) {
        __syncthreads();
        if (j0 + lane < cnt) {
            const pcr_pt r = recs[base + j0 + lane];
            s_c[0][lane] = r.x; s_c[1][lane] = r.y; s_c[2][lane] = r.z;
            mn[0] = r.x < mn[0] ? r.x : mn[0]; mn[1] = r.y < mn[1] ? r.y : mn[1]; mn[2] = r.z < mn[2] ? r.z : mn[2];
            ng[0] = -r.x < ng[0] ? -r.x : ng[0]; ng[1] = -r.y < ng[1] ? -r.y : ng[1]; ng[2] = -r.z < ng[2] ? -r.z : ng[2];
        }
        __syncthreads();
        const int nj = min(OB_WAVE, cnt - j0);
        if (lane < 3)
            for (int k = 0; k < nj; ++k) sum += s_c[lane][k];
    }
    double* const out = stats + 9 * o;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double lo = wave_min_f64(mn[a]), hi = -wave_min_f64(ng[a]);
        if (lane == 0) { out[3 + a] = lo; out[6 + a] = hi; }
    }
    if (lane < 3) out[lane] = sum / (double)cnt;
}

// One block.  tiles of object o: ceil(count / 64) if kept.  Objects are dealt to 32 classes by the power of two of their count, the
// class of the largest counts first; within a class the order is that of arrival (it decides only which tile starts first).
__global__ void __launch_bounds__(OB_BLOCK)
objects_tiles_kernel(const long long* __restrict__ off, const unsigned char* __restrict__ keep, int n_objects, ob_tile* __restrict__ tiles, unsigned int n_tiles) {
    __shared__ unsigned int s_total[32], s_base[32], s_cursor[32];
    if (threadIdx.x < 32) { s_total[threadIdx.x] = 0u; s_cursor[threadIdx.x] = 0u; }
    __syncthreads();
    auto tiles_of = [&](int o, int* cls) -> unsigned int {
        const long long cnt = off[o + 1] - off[o];
        if (cnt <= 0 || (keep && !keep[o])) return 0u;
        *cls = 31 - __clz((int)cnt);
        return (unsigned int)((cnt + OB_WAVE - 1) / OB_WAVE);
    };
    for (int o = threadIdx.x; o < n_objects; o += OB_BLOCK) {
        int cls = 0;
        const unsigned int t = tiles_of(o, &cls);
        if (t) atomicAdd(&s_total[cls], t);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned int run = 0u;
        for (int c = 31; c >= 0; --c) { s_base[c] = run; run += s_total[c]; }
    }
    __syncthreads();
    for (int o = threadIdx.x; o < n_objects; o += OB_BLOCK) {
        int cls = 0;
        const unsigned int t = tiles_of(o, &cls);
        if (!t) continue;
        const unsigned int first = s_base[cls] + atomicAdd(&s_cursor[cls], t);
        for (unsigned int k = 0; k < t; ++k)
            if (first + k < n_tiles) tiles[first + k] = ob_tile{o, (int)k};   // (the host counted the same tiles)
    }
}

// detect.py:299-301 for the 64 rows of one tile: w_i = (sum over j = 0 .. n-1, ascending, of d_ij) / n with
// d_ij = sqrt(((dx*dx) + dy*dy) + dz*dz), dx = x_i - x_j, the diagonal's +0.0 included -- pdist's distance and NumPy's column sum.
// Every lane reads the same staged j: LDS broadcasts, no bank conflict.
__global__ void __launch_bounds__(OB_WAVE)
objects_weights_kernel(const pcr_pt* __restrict__ recs, const long long* __restrict__ off, const ob_tile* __restrict__ tiles, int n_objects,
                       double* __restrict__ w) {
    __shared__ double s_x[OB_J], s_y[OB_J], s_z[OB_J];
    const int lane = threadIdx.x;
    const ob_tile t = tiles[blockIdx.x];
    if (t.object < 0 || t.object >= n_objects) return;   // (a slot the list kernel did not fill: the list was all ones before it ran)
    const long long base = off[t.object];
    const int cnt = (int)(off[t.object + 1] - base);
    const int i = t.iblock * OB_WAVE + lane;
    double xi = 0.0, yi = 0.0, zi = 0.0;
    if (i < cnt) { const pcr_pt r = recs[base + i]; xi = r.x; yi = r.y; zi = r.z; }
    double sum = 0.0;
    for (int j0 = 0; j0 < cnt; j0 += OB_J) {
        __syncthreads();
#pragma unroll
        for (int k = lane; k < OB_J; k += OB_WAVE)
            if (j0 + k < cnt) { const pcr_pt r = recs[base + j0 + k]; s_x[k] = r.x; s_y[k] = r.y; s_z[k] = r.z; }
        __syncthreads();
        const int nj = min(OB_J, cnt - j0);
#pragma unroll 4
        for (int k = 0; k < nj; ++k) {
            const double dx = xi - s_x[k], dy = yi - s_y[k], dz = zi - s_z[k];
            sum += sqrt((dx * dx + dy * dy) + dz * dz);
        }
    }
    if (i < cnt) w[base + i] = sum / (double)cnt;
}

__global__ void __launch_bounds__(OB_BLOCK)
objects_rows_kernel(const pcr_pt* __restrict__ recs, long long m, int* __restrict__ rows) {
    const long long k = (long long)blockIdx.x * OB_BLOCK + threadIdx.x;
    if (k < m) rows[k] = (int)recs[k].id;
}

// detect.py:311-318 then .float(): channels 0..2 = (float)(x - mean_o) subtracted in binary64, channels 3..5 = (float)normal of the row
__global__ void __launch_bounds__(OB_BLOCK)
objects_pack_kernel(const pcr_pt* __restrict__ recs, const long long* __restrict__ off, const double* __restrict__ stats, const double* __restrict__ normals,
                    const int* __restrict__ slot_object, const long long* __restrict__ local_idx, long long total, int S, float* __restrict__ out) {
    const long long e = (long long)blockIdx.x * OB_BLOCK + threadIdx.x;
    if (e >= total) return;
    const int o = slot_object[e / S];
    const pcr_pt r = recs[off[o] + local_idx[e]];
    const double* const mean = stats + 9 * (long long)o;
    float* const dst = out + e * (normals ? 6 : 3);
    dst[0] = (float)(r.x - mean[0]); dst[1] = (float)(r.y - mean[1]); dst[2] = (float)(r.z - mean[2]);
    if (normals) {
        const double* const nr = normals + 3 * r.id;
        dst[3] = (float)nr[0]; dst[4] = (float)nr[1]; dst[5] = (float)nr[2];
    }
}

// ---------------------------------------------------------------- KITTI boxes (detect.py:37-54 and :106-163)
constexpr int KB_ROWS = PCR_KITTI_LDS_ROWS;
static_assert(KB_ROWS % OB_WAVE == 0 && 3 * KB_ROWS * sizeof(double) <= 64 * 1024, "the camera-frame rows of one object, a whole number of wave loads");

// The heading direction of the x-z covariance [[a, b], [b, c]] as detect.py:47-54 reads it off np.linalg.eig (include/pcr.h has the
// derivation).  One source for pcr_kitti_direction and for the kernel.
__host__ __device__ inline void kitti_direction_rule(double a, double b, double c, double* cs, double* sn) {
    const double h = (a - c) * 0.5;
    if (b == 0.0) {
        if (h > 0.0) { *cs = 1.0; *sn = -0.0; }
        else { *cs = 0.0; *sn = -1.0; }
        return;
    }
    const double r = sqrt(h * h + b * b);
    double e0, e1;
    if (h >= 0.0) { e0 = h + r; e1 = b; }
    else { e0 = -b; e1 = r - h; }
    const double len = sqrt(e0 * e0 + e1 * e1);
    *cs = e0 / len;
    *sn = e1 / len;
}

// One wave per object.  Rows go to lanes round robin (row j to lane j % 64), so every sum has the order of include/pcr.h whatever
// the launch looks like.  on_chip: pass 1 leaves the camera-frame rows in LDS and passes 2 and 3 read them back (each lane its own
// rows: no hand-off between lanes); otherwise the two passes load the records again and repeat kb_cam -- the same operations, the
// same bits.
__global__ void __launch_bounds__(OB_WAVE)
kitti_boxes_kernel(const pcr_pt* __restrict__ recs, const long long* __restrict__ off, const unsigned char* __restrict__ keep, kb_calib k,
                   double* __restrict__ boxes) {
    __shared__ double s_X[3][KB_ROWS];
    const int lane = threadIdx.x;
    const long long o = blockIdx.x;
    const long long base = off[o];
    const int cnt = (int)(off[o + 1] - base);
    double* const out = boxes + PCR_KITTI_BOX_DOUBLES * o;
    if (cnt <= 0 || (keep && !keep[o])) {
        if (lane < PCR_KITTI_BOX_DOUBLES) out[lane] = lane == 15 ? (double)cnt : __longlong_as_double(0x7ff8000000000000ll);
        return;
    }
    const bool on_chip = cnt <= KB_ROWS;
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    const double n = (double)cnt;

    // pass 1: camera frame, pixel box, coordinate sums
    double sum[3] = {0.0, 0.0, 0.0};
    double mn[2] = {inf, inf}, ng[2] = {inf, inf};
    for (int j = lane; j < cnt; j += OB_WAVE) {
        double X[3], q[3];
        kb_cam(k, recs[base + j], X);
        if (on_chip) { s_X[0][j] = X[0]; s_X[1][j] = X[1]; s_X[2][j] = X[2]; }
#pragma unroll
        for (int i = 0; i < 3; ++i) q[i] = ((k.P[4 * i] * X[0] + k.P[4 * i + 1] * X[1]) + k.P[4 * i + 2] * X[2]) + k.P[4 * i + 3];
        const double px = q[0] / q[2], py = q[1] / q[2];
        mn[0] = px < mn[0] ? px : mn[0]; mn[1] = py < mn[1] ? py : mn[1];
        ng[0] = -px < ng[0] ? -px : ng[0]; ng[1] = -py < ng[1] ? -py : ng[1];
        sum[0] += X[0]; sum[1] += X[1]; sum[2] += X[2];
    }
    double ctr[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) ctr[i] = wave_object_sum_f64(sum[i]) / n;
    const double left = wave_min_f64(mn[0]), top = wave_min_f64(mn[1]), right = -wave_min_f64(ng[0]), bottom = -wave_min_f64(ng[1]);

    // pass 2: centred x-z moments, then the direction in every lane
    double m[3] = {0.0, 0.0, 0.0};
    for (int j = lane; j < cnt; j += OB_WAVE) {
        double X[3];
        if (on_chip) { X[0] = s_X[0][j]; X[2] = s_X[2][j]; }
        else kb_cam(k, recs[base + j], X);
        const double d0 = X[0] - ctr[0], d2 = X[2] - ctr[2];
        m[0] += d0 * d0; m[1] += d0 * d2; m[2] += d2 * d2;
    }
    const double a = wave_object_sum_f64(m[0]) / n, b = wave_object_sum_f64(m[1]) / n, c = wave_object_sum_f64(m[2]) / n;
    double cs, sn;
    kitti_direction_rule(a, b, c, &cs, &sn);
    const double ms = -sn;   // sin(-ry)

    // pass 3: extents in the object frame (detect.py:135-163)
    double lo[3] = {inf, inf, inf}, hi[3] = {inf, inf, inf};   // hi: minimum of the negated coordinate
    for (int j = lane; j < cnt; j += OB_WAVE) {
        double X[3];
        if (on_chip) { X[0] = s_X[0][j]; X[1] = s_X[1][j]; X[2] = s_X[2][j]; }
        else kb_cam(k, recs[base + j], X);
        const double d0 = X[0] - ctr[0], d1 = X[1] - ctr[1], d2 = X[2] - ctr[2];
        const double v[3] = {cs * d0 - ms * d2, d1, ms * d0 + cs * d2};
#pragma unroll
        for (int i = 0; i < 3; ++i) { lo[i] = v[i] < lo[i] ? v[i] : lo[i]; hi[i] = -v[i] < hi[i] ? -v[i] : hi[i]; }
    }
    double ext[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) ext[i] = -wave_min_f64(hi[i]) - wave_min_f64(lo[i]);
    if (lane == 0) {
        out[0] = left; out[1] = top; out[2] = right; out[3] = bottom;
        out[4] = ext[1]; out[5] = ext[0]; out[6] = ext[2];
        out[7] = ctr[0]; out[8] = ctr[1]; out[9] = ctr[2];
        out[10] = cs; out[11] = sn;
        out[12] = a; out[13] = b; out[14] = c;
        out[15] = n;
    }
}

inline unsigned int ob_grid(long long n) { return (unsigned int)((n + OB_BLOCK - 1) / OB_BLOCK); }

}  // namespace

extern "C" {

int pcr_objects_free(pcr_ctx* ctx, pcr_objects* objs) {
    if (!objs) return PCR_OK;
    if (!ctx) return PCR_E_INVALID;
    pcr_dev_free(ctx, objs->recs);
    pcr_dev_free(ctx, objs->d_off);
    pcr_dev_free(ctx, objs->d_stats);
    delete objs;
    return PCR_OK;
}

int pcr_objects_build(pcr_ctx* ctx, const pcr_cloud* cloud, const int32_t* labels, int32_t n_objects, pcr_objects** out) try {
    if (out) *out = nullptr;
    if (!ctx || !cloud || !labels || !out || n_objects < 0) return PCR_E_INVALID;
    const long long n = cloud->n;
    if (n <= 0) return PCR_E_EMPTY;
    if (n > std::numeric_limits<int32_t>::max()) return PCR_E_UNSUPPORTED;
    pcr_owned<pcr_objects, pcr_objects_free> objs(ctx, new pcr_objects());
    objs->n = n;
    objs->n_objects = n_objects;
    objs->off.assign((size_t)n_objects + 1, 0);
    for (long long i = 0; i < n; ++i) {
        if (labels[i] >= n_objects) return PCR_E_INVALID;
        if (labels[i] >= 0) objs->off[(size_t)labels[i] + 1] += 1;
    }
    for (int32_t o = 0; o < n_objects; ++o) objs->off[(size_t)o + 1] += objs->off[(size_t)o];
    const long long m = objs->m = objs->off[(size_t)n_objects];
    hipSetDevice(ctx->device);

    pcr_dev_block b_recs(ctx), b_off(ctx), b_stats(ctx), b_lab(ctx), b_k0(ctx), b_k1(ctx), b_v0(ctx), b_v1(ctx), b_temp(ctx);
    int rc;
    if ((rc = b_recs.alloc(sizeof(pcr_pt) * m)) || (rc = b_off.alloc(sizeof(long long) * ((size_t)n_objects + 1))) ||
        (rc = b_stats.alloc(sizeof(double) * 9 * (size_t)n_objects)))
        return rc;
    static_assert(sizeof(long long) == sizeof(int64_t), "offsets are uploaded as they are");
    PCR_HIP(ctx, hipMemcpyAsync(b_off.p, objs->off.data(), sizeof(long long) * ((size_t)n_objects + 1), hipMemcpyHostToDevice, ctx->stream));
    if (m > 0) {
        if ((rc = b_lab.alloc(sizeof(int) * n)) || (rc = b_k0.alloc(sizeof(unsigned int) * n)) || (rc = b_k1.alloc(sizeof(unsigned int) * n)) ||
            (rc = b_v0.alloc(sizeof(unsigned int) * n)) || (rc = b_v1.alloc(sizeof(unsigned int) * n)))
            return rc;
        PCR_HIP(ctx, hipMemcpyAsync(b_lab.p, labels, sizeof(int) * n, hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(objects_keys_kernel, dim3(ob_grid(n)), dim3(OB_BLOCK), 0, ctx->stream, b_lab.as<const int>(), n, (unsigned int)n_objects,
                           b_k0.as<unsigned int>(), b_v0.as<unsigned int>());
        PCR_HIP(ctx, hipGetLastError());
        unsigned int end_bit = 1;
        while (end_bit < 32 && ((unsigned int)n_objects >> end_bit)) ++end_bit;
        if ((rc = pcr_sort_pairs_arena(ctx, b_k0.as<unsigned int>(), b_k1.as<unsigned int>(), b_v0.as<unsigned int>(), b_v1.as<unsigned int>(), (size_t)n, end_bit,
                                       b_temp)))
            return rc;
        int* const d_dst = b_v0.as<int>();   // (the sort has read its input: stream order)
        PCR_HIP(ctx, hipMemsetAsync(d_dst, 0xff, sizeof(int) * n, ctx->stream));
        hipLaunchKernelGGL(objects_dst_kernel, dim3(ob_grid(m)), dim3(OB_BLOCK), 0, ctx->stream, b_v1.as<const unsigned int>(), m, d_dst);
        PCR_HIP(ctx, hipGetLastError());
        hipLaunchKernelGGL(objects_scatter_kernel, dim3(ob_grid(n)), dim3(OB_BLOCK), 0, ctx->stream, (const pcr_pt*)cloud->d, n, (const int*)d_dst, m,
                           b_recs.as<pcr_pt>());
        PCR_HIP(ctx, hipGetLastError());
    }
    if (n_objects > 0) {
        hipLaunchKernelGGL(objects_stats_kernel, dim3((unsigned int)n_objects), dim3(OB_WAVE), 0, ctx->stream, b_recs.as<const pcr_pt>(), b_off.as<const long long>(),
                           b_stats.as<double>());
        PCR_HIP(ctx, hipGetLastError());
    }
    PCR_HIP(ctx, pcr_sync(ctx->stream));   // the scratch of this call goes back to the arena, and `labels` is the caller's again
    objs->recs = b_recs.release<pcr_pt>();
    objs->d_off = b_off.release<long long>();
    objs->d_stats = b_stats.release<double>();
    *out = objs.release();
    return PCR_OK;
} PCR_CATCH(ctx)

int pcr_objects_offsets(const pcr_objects* objs, int64_t* offsets) {
    if (!objs || !offsets) return PCR_E_INVALID;
    memcpy(offsets, objs->off.data(), sizeof(int64_t) * objs->off.size());
    return PCR_OK;
}

int pcr_objects_rows(pcr_ctx* ctx, const pcr_objects* objs, int32_t* rows) {
    if (!ctx || !objs || !rows) return PCR_E_INVALID;
    const long long m = objs->m;
    if (m == 0) return PCR_OK;
    hipSetDevice(ctx->device);
    pcr_dev_block b_rows(ctx);
    int rc;
    if ((rc = b_rows.alloc(sizeof(int) * m))) return rc;
    hipLaunchKernelGGL(objects_rows_kernel, dim3(ob_grid(m)), dim3(OB_BLOCK), 0, ctx->stream, (const pcr_pt*)objs->recs, m, b_rows.as<int>());
    PCR_HIP(ctx, hipGetLastError());
    return pcr_d2h_staged(ctx, rows, b_rows.p, sizeof(int) * m);
}

int pcr_objects_stats(pcr_ctx* ctx, const pcr_objects* objs, int64_t* count, double* mean, double* bmin, double* bmax) try {
    if (!ctx || !objs) return PCR_E_INVALID;
    const size_t k = (size_t)objs->n_objects;
    if (count)
        for (size_t o = 0; o < k; ++o) count[o] = objs->off[o + 1] - objs->off[o];
    if (k == 0 || (!mean && !bmin && !bmax)) return PCR_OK;
    hipSetDevice(ctx->device);
    std::vector<double> h(9 * k);
    int rc;
    if ((rc = pcr_d2h_staged(ctx, h.data(), objs->d_stats, sizeof(double) * 9 * k))) return rc;
    for (size_t o = 0; o < k; ++o)
        for (int a = 0; a < 3; ++a) {
            if (mean) mean[3 * o + a] = h[9 * o + a];
            if (bmin) bmin[3 * o + a] = h[9 * o + 3 + a];
            if (bmax) bmax[3 * o + a] = h[9 * o + 6 + a];
        }
    return PCR_OK;
} PCR_CATCH(ctx)

int pcr_objects_select(const int64_t* count, const double* mean, int32_t n_objects, int64_t min_count, double max_radius, uint8_t* keep) {
    if (n_objects < 0 || (n_objects > 0 && (!count || !mean || !keep))) return PCR_E_INVALID;
    for (int32_t o = 0; o < n_objects; ++o) {
        const double mx = mean[3 * o], my = mean[3 * o + 1];
        const double r = sqrt(mx * mx + my * my);   // detect.py:291
        keep[o] = (count[o] > min_count && r <= max_radius) ? 1 : 0;   // (a NaN centre fails the comparison: dropped)
    }
    return PCR_OK;
}

int pcr_objects_weights(pcr_ctx* ctx, const pcr_objects* objs, const uint8_t* keep, double* weights) {
    if (!ctx || !objs || !weights) return PCR_E_INVALID;
    const long long m = objs->m;
    const int n_objects = (int)objs->n_objects;
    if (m == 0) return PCR_OK;
    long long n_tiles = 0;
    for (int o = 0; o < n_objects; ++o)
        if (!keep || keep[o]) n_tiles += (objs->off[(size_t)o + 1] - objs->off[(size_t)o] + OB_WAVE - 1) / OB_WAVE;
    if (n_tiles > std::numeric_limits<int32_t>::max()) return PCR_E_UNSUPPORTED;
    if (n_tiles == 0) { memset(weights, 0, sizeof(double) * m); return PCR_OK; }
    hipSetDevice(ctx->device);
    pcr_dev_block b_w(ctx), b_tiles(ctx), b_keep(ctx);
    int rc;
    if ((rc = b_w.alloc(sizeof(double) * m)) || (rc = b_tiles.alloc(sizeof(ob_tile) * n_tiles))) return rc;
    if (keep) {
        if ((rc = b_keep.alloc((size_t)n_objects))) return rc;
        PCR_HIP(ctx, hipMemcpyAsync(b_keep.p, keep, (size_t)n_objects, hipMemcpyHostToDevice, ctx->stream));
    }
    PCR_HIP(ctx, hipMemsetAsync(b_w.p, 0, sizeof(double) * m, ctx->stream));   // rows of unselected objects
    PCR_HIP(ctx, hipMemsetAsync(b_tiles.p, 0xff, sizeof(ob_tile) * n_tiles, ctx->stream));
    hipLaunchKernelGGL(objects_tiles_kernel, dim3(1), dim3(OB_BLOCK), 0, ctx->stream, (const long long*)objs->d_off, b_keep.as<const unsigned char>(), n_objects,
                       b_tiles.as<ob_tile>(), (unsigned int)n_tiles);
    PCR_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(objects_weights_kernel, dim3((unsigned int)n_tiles), dim3(OB_WAVE), 0, ctx->stream, (const pcr_pt*)objs->recs, (const long long*)objs->d_off,
                       b_tiles.as<const ob_tile>(), n_objects, b_w.as<double>());
    PCR_HIP(ctx, hipGetLastError());
    return pcr_d2h_staged(ctx, weights, b_w.p, sizeof(double) * m);
}

int pcr_objects_pack_f32(pcr_ctx* ctx, const pcr_objects* objs, const double* normals, const int32_t* slot_object, const int64_t* local_idx, int64_t b, int64_t S,
                         void* out_device) {
    if (!ctx || !objs || b < 0 || S < 0) return PCR_E_INVALID;
    if (b == 0 || S == 0) return PCR_OK;
    if (!slot_object || !local_idx || !out_device || b > std::numeric_limits<int32_t>::max() || S > std::numeric_limits<int32_t>::max()) return PCR_E_INVALID;
    for (int64_t s = 0; s < b; ++s) {
        const int32_t o = slot_object[s];
        if (o < 0 || o >= objs->n_objects) return PCR_E_INVALID;
        const int64_t cnt = objs->off[(size_t)o + 1] - objs->off[(size_t)o];
        for (int64_t k = 0; k < S; ++k)
            if (local_idx[s * S + k] < 0 || local_idx[s * S + k] >= cnt) return PCR_E_INVALID;
    }
    const long long total = b * S;
    if (total > (long long)std::numeric_limits<int32_t>::max() * OB_BLOCK) return PCR_E_UNSUPPORTED;
    hipSetDevice(ctx->device);
    pcr_dev_block b_slot(ctx), b_idx(ctx), b_nrm(ctx);
    int rc;
    if ((rc = b_slot.alloc(sizeof(int) * b)) || (rc = b_idx.alloc(sizeof(long long) * total))) return rc;
    PCR_HIP(ctx, hipMemcpyAsync(b_slot.p, slot_object, sizeof(int) * b, hipMemcpyHostToDevice, ctx->stream));
    PCR_HIP(ctx, hipMemcpyAsync(b_idx.p, local_idx, sizeof(long long) * total, hipMemcpyHostToDevice, ctx->stream));
    if (normals) {
        if ((rc = b_nrm.alloc(sizeof(double) * 3 * objs->n))) return rc;
        PCR_HIP(ctx, hipMemcpyAsync(b_nrm.p, normals, sizeof(double) * 3 * objs->n, hipMemcpyHostToDevice, ctx->stream));
    }
    hipLaunchKernelGGL(objects_pack_kernel, dim3(ob_grid(total)), dim3(OB_BLOCK), 0, ctx->stream, (const pcr_pt*)objs->recs, (const long long*)objs->d_off,
                       (const double*)objs->d_stats, b_nrm.as<const double>(), b_slot.as<const int>(), b_idx.as<const long long>(), total, (int)S, (float*)out_device);
    PCR_HIP(ctx, hipGetLastError());
    PCR_HIP(ctx, pcr_sync(ctx->stream));   // the tensor is the caller's framework's from here on
    return PCR_OK;
}

int pcr_kitti_direction(double a, double b, double c, double* cs, double* sn) {
    if (!cs || !sn) return PCR_E_INVALID;
    kitti_direction_rule(a, b, c, cs, sn);
    return PCR_OK;
}

int pcr_objects_kitti_boxes(pcr_ctx* ctx, const pcr_objects* objs, const pcr_kitti_calib* calib, const uint8_t* keep, double* boxes) {
    if (!ctx || !objs || !calib || !boxes) return PCR_E_INVALID;
    kb_calib k;
    memcpy(k.T, calib->Tr_velo_to_cam, sizeof(k.T));
    memcpy(k.R0, calib->R0_rect, sizeof(k.R0));
    memcpy(k.P, calib->P2, sizeof(k.P));
    for (double v : k.T) if (!std::isfinite(v)) return PCR_E_INVALID;
    for (double v : k.R0) if (!std::isfinite(v)) return PCR_E_INVALID;
    for (double v : k.P) if (!std::isfinite(v)) return PCR_E_INVALID;
    const size_t n_objects = (size_t)objs->n_objects;
    if (n_objects == 0) return PCR_OK;
    hipSetDevice(ctx->device);
    pcr_dev_block b_boxes(ctx), b_keep(ctx);
    int rc;
    if ((rc = b_boxes.alloc(sizeof(double) * PCR_KITTI_BOX_DOUBLES * n_objects))) return rc;
    if (keep) {
        if ((rc = b_keep.alloc(n_objects))) return rc;
        PCR_HIP(ctx, hipMemcpyAsync(b_keep.p, keep, n_objects, hipMemcpyHostToDevice, ctx->stream));
    }
    hipLaunchKernelGGL(kitti_boxes_kernel, dim3((unsigned int)n_objects), dim3(OB_WAVE), 0, ctx->stream, (const pcr_pt*)objs->recs, (const long long*)objs->d_off,
                       b_keep.as<const unsigned char>(), k, b_boxes.as<double>());
    PCR_HIP(ctx, hipGetLastError());
    return pcr_d2h_staged(ctx, boxes, b_boxes.p, sizeof(double) * PCR_KITTI_BOX_DOUBLES * n_objects);   // (waits for the stream: `keep` is the caller's again)
}

}  // extern "C"
