// The walk over a point's radius neighbourhood that the ISS passes (pcr_iss.hip) and the Harris / PCL-rule passes (pcr_harris.hip)
// share: a grid with cell = radius, the 3x3x3 block of the point's cell, IG lanes per point, every lane owning the cells
// gl, gl + IG, ... of the 27.  A lane meets its cells in that order and a cell's records in stored order: a sum taken inside
// `f` runs in a fixed order.  Cells outside the representable range, or that the table does not hold, are empty.
#pragma once
#include <string>
#include "pcr_grid_dev.h"

constexpr int IG = 8;  // lanes per point

template <class F>
__device__ static inline void iss_visit_block(const pcr_grid_view& gv, double ax, double ay, double az, int gl, F& f) {
    bool clamped = false;
    const int cx = cell_coord(ax, gv.lo[0], gv.inv_cell0, &clamped);
    const int cy = cell_coord(ay, gv.lo[1], gv.inv_cell0, &clamped);
    const int cz = cell_coord(az, gv.lo[2], gv.inv_cell0, &clamped);
#pragma unroll
    for (int i = 0; i < (27 + IG - 1) / IG; ++i) {
        const int n = gl + i * IG;
        if (n < 27) {
            const unsigned int nx = (unsigned int)(cx + n % 3 - 1), ny = (unsigned int)(cy + (n / 3) % 3 - 1), nz = (unsigned int)(cz + n / 9 - 1);
            if (nx <= (unsigned int)PCR_COORD_MAX && ny <= (unsigned int)PCR_COORD_MAX && nz <= (unsigned int)PCR_COORD_MAX) {
                unsigned int s, e;
                if (lookup_cell(gv.table[0], gv.mask[0], nx, ny, nz, &s, &e))
                    for (unsigned int j0 = s; j0 < e; j0 += 4) {   // four records per trip, requested together
                        pcr_pt rec[4];
#pragma unroll
                        for (int u = 0; u < 4; ++u) {   // (assigned on every path: conditionally unassigned records become loop-carried registers)
                            rec[u] = pcr_pt{0.0, 0.0, 0.0, 0};
                            if (j0 + u < e) rec[u] = gv.pts[j0 + u];
                        }
#pragma unroll
                        for (int u = 0; u < 4; ++u)
                            if (j0 + u < e) f(rec[u]);
                    }
            }
        }
    }
}

// The lanes' partial sums of one point, combined in a fixed order (lane pairs 4 apart, then 2, then 1): every lane of the group ends
// with the same bits, whatever the launch.
__device__ static inline double ball_lanes_sum(double v) {
#pragma unroll
    for (int off = IG / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ static inline int ball_lanes_sum(int v) {
#pragma unroll
    for (int off = IG / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// (host) the grid whose 3x3x3 block covers a ball of `radius` and is of its size (pcr_iss's rule and refusal)
// The index sorts stably by cell, so a cell's records keep the order of the cloud's: a cloud that a search has laid out along its
// curve is indexed from a copy in caller-row order, and its sums then run in the very order of the cloud as uploaded (same bits).
static inline int ball_grid(pcr_ctx* ctx, const pcr_cloud* cloud, double radius, const char* who, pcr_index_guard& idx) {
    const double cell_req = radius * (1.0 + 1e-9);
    int rc;
    pcr_dev_block b_rows(ctx);
    pcr_cloud by_row = *cloud;
    if (cloud->morton_sorted) {
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
