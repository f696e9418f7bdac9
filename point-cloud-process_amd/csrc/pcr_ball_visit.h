// The walk over a radius ball, once: a grid with cell = radius (ball_grid), so the ball of a centre lies in the 3x3x3 block of the
// centre's cell.  Block cell c = 0..26 counts x fastest; a cell outside the representable range, or that the table does not hold, is
// empty.  Users:
//   pcr_iss.hip        both ISS passes                                        lane-group walk (grid over the cloud as stored)
//   pcr_harris.hip     position covariance, normal covariance, suppression    lane-group walk;  refine: wave walk
//   pcr_fpfh_pcl.hip   mark, SPFH, FPFH                                       wave walk, the last two with the ballot compaction
//   pcr_sift.hip       DoG pass, the 25 nearest rows of a candidate           wave walk
//   pcr_normals.hip    normals_kernel<K>                                      the cell lookup (its own cell size and its own loop, see there)
// (gather_hybrid of pcr_features.hip keeps its own cell lookup and ballot compaction beside its flat list: the note there says why.)
// Lane-group walk: BALL_LANES lanes per point, lane gl owns the cells gl, gl + LANES, ...; it meets them in that order and a cell's records
// in stored order.  Wave walk: one wave per centre, lanes 0..26 look one cell up each, the wave takes the 27 runs one after the other,
// 64 positions a trip, lane l meeting the records l, l + 64, ... of a run.  Either way a sum taken inside `f` runs in a fixed order.
#pragma once
#include <string>
#include "pcr_grid_dev.h"

constexpr int BALL_LANES = 8;  // lanes per point of the ISS and Harris passes

// ---------------------------------------------------------------- cell lookup
// the cell of (x, y, z); true: a coordinate was clamped (outside the representable range, or not finite)
__device__ static inline bool ball_centre_cell(const pcr_grid_view& gv, double x, double y, double z, int* ix, int* iy, int* iz) {
    bool clamped = false;
    *ix = cell_coord(x, gv.lo[0], gv.inv_cell0, &clamped);
    *iy = cell_coord(y, gv.lo[1], gv.inv_cell0, &clamped);
    *iz = cell_coord(z, gv.lo[2], gv.inv_cell0, &clamped);
    return clamped;
}
// the run [s, e) of the sorted cloud that is cell c of the block around cell (ix, iy, iz); false and s = e = 0: the cell is empty
__device__ static inline bool ball_cell_run(const pcr_grid_view& gv, int ix, int iy, int iz, int c, unsigned int* s, unsigned int* e) {
    *s = *e = 0;
    const unsigned int nx = (unsigned int)(ix + c % 3 - 1), ny = (unsigned int)(iy + (c / 3) % 3 - 1), nz = (unsigned int)(iz + c / 9 - 1);
    return nx <= (unsigned int)PCR_COORD_MAX && ny <= (unsigned int)PCR_COORD_MAX && nz <= (unsigned int)PCR_COORD_MAX &&
           lookup_cell(gv.table[0], gv.mask[0], nx, ny, nz, s, e);
}

// ---------------------------------------------------------------- lane-group walk
// f(record, position) for every record of the cells of lane gl
template <int LANES, class F>
__device__ static inline void ball_visit(const pcr_grid_view& gv, double ax, double ay, double az, int gl, F& f) {
    int cx, cy, cz;
    ball_centre_cell(gv, ax, ay, az, &cx, &cy, &cz);   // (a clamped centre walks the block of the clamped cell)
    constexpr int TRIPS = (27 + LANES - 1) / LANES;
#pragma unroll
    for (int i = 0; i < TRIPS; ++i) {
        const int c = gl + i * LANES;
        unsigned int s, e;
        if (c < 27 && ball_cell_run(gv, cx, cy, cz, c, &s, &e))
            for (unsigned int j0 = s; j0 < e; j0 += 4) {   // four records per trip, requested together
                pcr_pt rec[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {   // (assigned on every path: conditionally unassigned records become loop-carried registers)
                    rec[u] = pcr_pt{0.0, 0.0, 0.0, 0};
                    if (j0 + u < e) rec[u] = gv.pts[j0 + u];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (j0 + u < e) f(rec[u], j0 + u);
            }
    }
}

// This thread's point and lane in a launch of ball_blocks(n) blocks of 256 threads; false: there is no such point (the lanes of a
// point leave together)
__device__ static inline bool ball_lane_point(long long n, long long* i, int* gl) {
    *gl = threadIdx.x % BALL_LANES;
    *i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) / BALL_LANES;
    return *i < n;
}
static inline unsigned ball_blocks(int64_t n) { return (unsigned)((n * BALL_LANES + 255) / 256); }

// The lanes' partial sums of one point, combined in a fixed order (lane pairs 4 apart, then 2, then 1): every lane of the group ends
// with the same bits, whatever the launch.
__device__ static inline double ball_lanes_sum(double v) {
#pragma unroll
    for (int off = BALL_LANES / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ static inline int ball_lanes_sum(int v) {
#pragma unroll
    for (int off = BALL_LANES / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// ---------------------------------------------------------------- wave walk
// lanes 0..26: the run of cell `lane` of the block around (x, y, z); an empty run for the other lanes, for empty cells, and in every
// lane for a centre whose cell was clamped (a centre far outside the cloud, or not finite, meets no record at all)
__device__ static inline void wave_block_runs(const pcr_grid_view& gv, double x, double y, double z, int lane, unsigned int* s, unsigned int* e) {
    *s = *e = 0;
    int ix, iy, iz;
    if (lane < 27 && !ball_centre_cell(gv, x, y, z, &ix, &iy, &iz)) ball_cell_run(gv, ix, iy, iz, lane, s, e);
}
// f(position, valid) by the whole wave, once per trip of 64 positions of each of the 27 runs in order: lane l gets position
// j0 + l, valid while it is inside the run.  Every lane takes part in every trip, so `f` may ballot.
template <class F>
__device__ static inline void wave_visit_runs(unsigned int s, unsigned int e, int lane, F& f) {
    for (int cell = 0; cell < 27; ++cell) {
        const unsigned int cs = __shfl(s, cell, 64), ce = __shfl(e, cell, 64);
        for (unsigned int j0 = cs; j0 < ce; j0 += 64) f(j0 + lane, j0 + lane < ce);
    }
}
// ballot compaction: the rank of this lane's `in` among the lanes below it, and how many lanes of the wave have it set
__device__ static inline int wave_compact_slot(bool in, int lane, int* added) {
    const unsigned long long mask = __ballot(in);
    *added = __popcll(mask);
    return __popcll(mask & ((1ull << lane) - 1ull));
}

// ---------------------------------------------------------------- (host) the grid
// The grid whose 3x3x3 block covers a ball of `radius` and is of its size.  The index keeps 2^18 level-0 cells per axis and coarsens
// the cell of a cloud whose extent is more than 2^18 radii: the block would still cover the ball, but no longer be of its size, and a
// pass would read every point of 27 cells many radii wide.  That is refused.
// The index sorts stably by cell, so a cell's records keep the order of the cloud's.  as_stored = false: a cloud that a search has laid
// out along its curve is indexed from a copy in caller-row order, and its sums then run in the very order of the cloud as uploaded (same
// bits).  as_stored = true (pcr_iss): the cloud is indexed in the order it has on the device.
static inline int ball_grid(pcr_ctx* ctx, const pcr_cloud* cloud, double radius, const char* who, pcr_index_guard& idx, bool as_stored = false) {
    const double cell_req = radius * (1.0 + 1e-9);   // the block of 27 cells covers the ball with rounding slack
    int rc;
    pcr_dev_block b_rows(ctx);
    pcr_cloud by_row = *cloud;
    if (cloud->morton_sorted && !as_stored) {
        if ((rc = b_rows.alloc(sizeof(pcr_pt) * cloud->n)) || (rc = pcr_cloud_rows(ctx, cloud, b_rows.as<pcr_pt>()))) return rc;
        by_row.d = b_rows.as<pcr_pt>();
        by_row.morton_sorted = false;
    }
    if ((rc = pcr_index_build(ctx, &by_row, PCR_INDEX_GRID, cell_req, &idx.h))) return rc;
    if (idx->cell > cell_req || idx->cell < radius * (1.0 - 1e-12)) {
        ctx->last_error = std::string(who) + ": the cloud's extent exceeds 2^18 radii; the grid cannot hold a cell of the radius";
        return PCR_E_UNSUPPORTED;
    }
    return PCR_OK;
}
