// The KITTI calibration as the kernels take it and the camera-frame transform of one row: shared by the boxes (pcr_objects.hip) and the
// label match (pcr_label_match.hip), so that both run the one written order of include/pcr.h.
#pragma once
#include "pcr_internal.h"

struct kb_calib { double T[12], R0[9], P[12]; };   // row-major: Tr_velo_to_cam, R0_rect, P2

// transform_to_cam (transform_coords_utils.py:4-32) of one row
__device__ static inline void kb_cam(const kb_calib& k, const pcr_pt& r, double (&X)[3]) {
    double u[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) u[i] = ((k.T[4 * i] * r.x + k.T[4 * i + 1] * r.y) + k.T[4 * i + 2] * r.z) + k.T[4 * i + 3];
#pragma unroll
    for (int i = 0; i < 3; ++i) X[i] = (k.R0[3 * i] * u[0] + k.R0[3 * i + 1] * u[1]) + k.R0[3 * i + 2] * u[2];
}
