// The Darboux frame of a pair of oriented points and the bin rule of the 11-bin histograms -- the one copy that the Open3D-rule
// SPFH (pcr_features.hip: spfh_body) and the PCL-rule SPFH (pcr_fpfh_pcl.hip) share.
#pragma once
#include <cmath>

// Darboux-frame pair features (Open3D ComputePairFeatures): f0 = atan2 angle, f1 = v.n2, f2 = n1.d/|d|
// Returns false for a degenerate pair -- zero length, or a zero cross product -- with f as Open3D's Zero() return leaves it: the
// Open3D rule bins such a pair all the same (bins 5, 5, 5 or 5, 5, f2's), the PCL rule skips it.
__device__ static inline bool pair_features(const double p1[3], const double n1[3], const double p2[3], const double n2[3], double f[3]) {
    double d[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
    const double len = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    f[0] = f[1] = f[2] = 0.0;
    if (len == 0.0) return false;  // zero vector still lands in bins (5, 5, 5), like Open3D's Zero() return
    const double a1 = ((n1[0] * d[0] + n1[1] * d[1]) + n1[2] * d[2]) / len;
    const double a2 = ((n2[0] * d[0] + n2[1] * d[1]) + n2[2] * d[2]) / len;
    double u[3], w2[3];
    if (fabs(a1) < fabs(a2)) {  // acos(|a1|) > acos(|a2|): the frame is anchored at the point whose normal is closer to the line
        u[0] = n2[0]; u[1] = n2[1]; u[2] = n2[2];
        w2[0] = n1[0]; w2[1] = n1[1]; w2[2] = n1[2];
        d[0] = -d[0]; d[1] = -d[1]; d[2] = -d[2];
        f[2] = -a2;
    } else {
        u[0] = n1[0]; u[1] = n1[1]; u[2] = n1[2];
        w2[0] = n2[0]; w2[1] = n2[1]; w2[2] = n2[2];
        f[2] = a1;
    }
    double v[3] = {d[1] * u[2] - d[2] * u[1], d[2] * u[0] - d[0] * u[2], d[0] * u[1] - d[1] * u[0]};
    const double vn = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    if (vn == 0.0) { f[2] = 0.0; return false; }
    v[0] /= vn; v[1] /= vn; v[2] /= vn;
    const double w[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
    f[1] = (v[0] * w2[0] + v[1] * w2[1]) + v[2] * w2[2];
    f[0] = atan2((w[0] * w2[0] + w[1] * w2[1]) + w[2] * w2[2], (u[0] * w2[0] + u[1] * w2[1]) + u[2] * w2[2]);
    return true;
}

__device__ static inline int clamp_bin(double x) {
    int h = (int)floor(x);
    return h < 0 ? 0 : (h > 10 ? 10 : h);
}

// the three bins (of 33: blocks of 11) that a pair's features fall into
__device__ static inline void pair_bins(const double f[3], int bins[3]) {
    bins[0] = clamp_bin(11.0 * (f[0] + M_PI) / (2.0 * M_PI));
    bins[1] = 11 + clamp_bin(11.0 * (f[1] + 1.0) * 0.5);
    bins[2] = 22 + clamp_bin(11.0 * (f[2] + 1.0) * 0.5);
}
