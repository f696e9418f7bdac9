// The nested cell hierarchy as the exact descents walk it (the 1-NN hard stage of pcr_grid_search.hip, the k-NN and radius
// kernels of pcr_knn.hip): the entry of a stack of cells still to split and the distance from a query to a cell's box.
#pragma once
#include "pcr_grid_dev.h"

struct cell_entry {   // a cell on a descent's stack: its run of the Morton-sorted target and its integer coordinates at `level`
    unsigned int start, end;
    unsigned int x, y, z;
    int level;
};

__device__ static inline double sq_pos(double v) {
    v = fmax(v, 0.0);
    return v * v;
}

// squared distance from (ax, ay, az) to the box of cell (X, Y, Z) of `level` (edge `cell`), rounded DOWN by a slack: only ever a prune test
__device__ static inline double box_dist2(const pcr_grid_view& gv, int level, double cell, unsigned int X, unsigned int Y, unsigned int Z,
                                          double ax, double ay, double az) {
    const int bl = (int)(PCR_COORD_BIAS >> (2 * level));
    const double slack = cell * 1e-9;
    const double x0 = gv.lo[0] + (double)((int)X - bl) * cell;
    const double y0 = gv.lo[1] + (double)((int)Y - bl) * cell;
    const double z0 = gv.lo[2] + (double)((int)Z - bl) * cell;
    const double dx = sq_pos(fmax(x0 - ax, ax - (x0 + cell)) - slack);
    const double dy = sq_pos(fmax(y0 - ay, ay - (y0 + cell)) - slack);
    const double dz = sq_pos(fmax(z0 - az, az - (z0 + cell)) - slack);
    return (dx + dy) + dz;
}
