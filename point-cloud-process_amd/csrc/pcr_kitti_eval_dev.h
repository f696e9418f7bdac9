// The box overlaps of the KITTI evaluation (include/pcr.h, "KITTI evaluation"): ONE source for the overlap kernel and for the host's
// pcr_kitti_box_overlap, and plain C++ besides, so that a stand-alone host program can be built from it with a sanitizer and without
// the HIP runtime.  Everything is binary64 in the written order (the library is compiled without contraction); cos(ry) and sin(ry)
// are the caller's: no transcendental runs here.
// The clip keeps a polygon of at most 8 vertices in fixed-size arrays that are only ever indexed by constants: a vertex is appended by
// eight selects on (count == k) instead of a store at a computed position, so on the device the arrays stay in registers.
#pragma once

#if defined(__HIPCC__)
#define KE_HD __host__ __device__
#else
#define KE_HD
#endif

struct ke_box { double left, top, right, bottom, h, w, l, cx, cy, cz, cs, sn; };

KE_HD static inline bool ke_finite(double v) { return v - v == 0.0; }   // false for NaN and for +-inf

// a row of 16 doubles in KITTI_COLUMNS order, with the caller's cos(ry), sin(ry)
KE_HD static inline ke_box ke_box_from_row(const double* r, double cs, double sn) {
    ke_box b;
    b.left = r[4]; b.top = r[5]; b.right = r[6]; b.bottom = r[7];
    b.h = r[8]; b.w = r[9]; b.l = r[10];
    b.cx = r[11]; b.cy = r[12]; b.cz = r[13];
    b.cs = cs; b.sn = sn;
    return b;
}

struct ke_poly { double x[8], z[8]; int n; };

KE_HD static inline void ke_put(ke_poly& o, bool flag, double vx, double vz) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const bool here = flag && o.n == k;
        o.x[k] = here ? vx : o.x[k];
        o.z[k] = here ? vz : o.z[k];
    }
    o.n += flag ? 1 : 0;
}

// The part of the convex polygon p (at most NIN vertices, counter-clockwise) on or to the left of the line P -> Q.  The side of every
// vertex is computed once, s = ex*(z - pz) - ez*(x - px) with e = Q - P, and s >= 0 is inside; an edge whose ends differ in side adds
// V_i + t*(V_j - V_i), t = s_i / (s_i - s_j).  A convex polygon gains at most one vertex per line, so 8 slots hold a quad after four
// lines; should rounding ever produce a sign pattern with more crossings, the vertices beyond the eighth are dropped.
template <int NIN>
KE_HD static inline void ke_clip(const ke_poly& p, double px, double pz, double qx, double qz, ke_poly& o) {
    const double ex = qx - px, ez = qz - pz;
    double s[NIN];
#pragma unroll
    for (int i = 0; i < NIN; ++i) s[i] = ex * (p.z[i] - pz) - ez * (p.x[i] - px);
    o.n = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) { o.x[k] = 0.0; o.z[k] = 0.0; }
#pragma unroll
    for (int i = 0; i < NIN; ++i) {
        const int j = i + 1 < NIN ? i + 1 : 0;           // (a constant after unrolling)
        const bool last = !(i + 1 < p.n);                 // the vertex after the last one is the first
        const double nx = last ? p.x[0] : p.x[j], nz = last ? p.z[0] : p.z[j], ns = last ? s[0] : s[j];
        const bool live = i < p.n;
        const bool in_i = s[i] >= 0.0, in_j = ns >= 0.0;
        const bool cross = live && in_i != in_j;
        const double den = cross ? s[i] - ns : 1.0;       // (signs differ: never zero)
        const double t = s[i] / den;
        ke_put(o, live && in_i, p.x[i], p.z[i]);
        ke_put(o, cross, p.x[i] + t * (nx - p.x[i]), p.z[i] + t * (nz - p.z[i]));
    }
    o.n = o.n < 8 ? o.n : 8;
}

// corner k = 0..3 of a box, local (x, z) = (+, +), (-, +), (-, -), (+, -) halves of (l, w): counter-clockwise, and the map has
// determinant cs*cs + sn*sn, so both quads keep that orientation
KE_HD static inline void ke_corner(const ke_box& b, int k, double ox, double oz, double& X, double& Z) {
    const double hx = b.l * 0.5, hz = b.w * 0.5;
    const double x = (k == 0 || k == 3) ? hx : -hx;
    const double z = (k == 0 || k == 1) ? hz : -hz;
    X = (b.cs * x + b.sn * z) + ox;
    Z = (b.cs * z - b.sn * x) + oz;
}

// area of the intersection of the two ground rectangles: b's quad, relative to a's centre, clipped by the four edges of a's
KE_HD static inline double ke_ground_intersection(const ke_box& a, const ke_box& b) {
    const double dx = b.cx - a.cx, dz = b.cz - a.cz;
    double ax[4], az[4];
    ke_poly p0, p1;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        ke_corner(a, k, 0.0, 0.0, ax[k], az[k]);
        ke_corner(b, k, dx, dz, p0.x[k], p0.z[k]);
    }
#pragma unroll
    for (int k = 4; k < 8; ++k) { p0.x[k] = 0.0; p0.z[k] = 0.0; }
    p0.n = 4;
    ke_clip<4>(p0, ax[0], az[0], ax[1], az[1], p1);
    ke_clip<5>(p1, ax[1], az[1], ax[2], az[2], p0);
    ke_clip<6>(p0, ax[2], az[2], ax[3], az[3], p1);
    ke_clip<7>(p1, ax[3], az[3], ax[0], az[0], p0);
    double twice = 0.0;   // shoelace in vertex order
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int j = i + 1 < 8 ? i + 1 : 0;
        const bool last = !(i + 1 < p0.n);
        const double nx = last ? p0.x[0] : p0.x[j], nz = last ? p0.z[0] : p0.z[j];
        const double term = p0.x[i] * nz - nx * p0.z[i];
        twice = i < p0.n ? twice + term : twice;
    }
    const double area = 0.5 * twice;
    return (p0.n >= 3 && area > 0.0) ? area : 0.0;
}

KE_HD static inline double ke_ratio(double inter, double a, double b, int criterion) {
    const double den = criterion < 0 ? (a + b) - inter : (criterion == 0 ? a : b);
    return inter / den;
}

// out[0] image, out[1] ground, out[2] 3-D; criterion -1 union, 0 the first box, 1 the second
KE_HD static inline void ke_overlaps(const ke_box& a, const ke_box& b, int criterion, double out[3]) {
    out[0] = 0.0; out[1] = 0.0; out[2] = 0.0;
    if (ke_finite(a.left) && ke_finite(a.top) && ke_finite(a.right) && ke_finite(a.bottom) && ke_finite(b.left) && ke_finite(b.top) && ke_finite(b.right) &&
        ke_finite(b.bottom)) {
        const double w = (a.right < b.right ? a.right : b.right) - (a.left > b.left ? a.left : b.left);
        const double h = (a.bottom < b.bottom ? a.bottom : b.bottom) - (a.top > b.top ? a.top : b.top);
        if (w > 0.0 && h > 0.0)
            out[0] = ke_ratio(w * h, (a.right - a.left) * (a.bottom - a.top), (b.right - b.left) * (b.bottom - b.top), criterion);
    }
    const bool ground_ok = ke_finite(a.w) && ke_finite(a.l) && ke_finite(a.cx) && ke_finite(a.cz) && ke_finite(a.cs) && ke_finite(a.sn) && ke_finite(b.w) &&
                           ke_finite(b.l) && ke_finite(b.cx) && ke_finite(b.cz) && ke_finite(b.cs) && ke_finite(b.sn) && a.l > 0.0 && a.w > 0.0 && b.l > 0.0 &&
                           b.w > 0.0;
    if (!ground_ok) return;
    const double inter = ke_ground_intersection(a, b);
    if (!(inter > 0.0)) return;
    out[1] = ke_ratio(inter, a.l * a.w, b.l * b.w, criterion);
    if (!(ke_finite(a.h) && ke_finite(a.cy) && ke_finite(b.h) && ke_finite(b.cy) && a.h > 0.0 && b.h > 0.0)) return;
    const double top_a = a.cy - a.h, top_b = b.cy - b.h;
    const double hh = (a.cy < b.cy ? a.cy : b.cy) - (top_a > top_b ? top_a : top_b);
    if (hh > 0.0) out[2] = ke_ratio(inter * hh, (a.h * a.l) * a.w, (b.h * b.l) * b.w, criterion);
}
