// The lay-out curve of a QUERY cloud (pcr_cloud_morton_sort): which 32 records form a wave tile of the ICP pass.  The target's
// order must be Morton (the index's tables need its nested-octree property); a query cloud's order is free, and every sum of the
// pass is an order-independent integer sum, so the curve changes which candidates a tile stages and nothing of the result.  A Z
// curve jumps -- a run of 32 that crosses a high-order bit boundary joins two far-apart clumps, and the tile's box holds everything
// in between; a Hilbert curve never does: cells of consecutive keys are face neighbours.
//
// Both keys are over the cloud's own box, like morton_key: origin `lo`, 1 / cell `inv`, cell_coord's clamping, and the low `nb`
// bits of every cell coordinate (nb = pcr_morton_end_bit / 3), so a key is as wide as the Morton key it replaces.  Set-up code, once
// per cloud: plain loops over the levels (Skilling's transpose algorithm, "Programming the Hilbert curve", 2004).
#pragma once
#include "pcr_grid_dev.h"

enum { PCR_CURVE_MORTON = 0, PCR_CURVE_HILBERT3 = 1, PCR_CURVE_HILBERT2_MINOR = 2 };

struct pcr_curve {   // chosen on the host from the cloud's box (pcr_curve_pick), a kernel argument
    int mode;        // PCR_CURVE_*
    int nb;          // bits per axis of the Hilbert index
    int ax[3];       // HILBERT2_MINOR: the curve runs over axes ax[0], ax[1]; ax[2] is the minor key
    int nb_minor;    // HILBERT2_MINOR: bits of the minor axis' cell coordinate
    int bits;        // width of the key
};

// Hilbert index of the N coordinates X[0..N) of `nb` bits each (X is overwritten); X[0] holds the most significant bit
template <int N>
__host__ __device__ static inline unsigned long long hilbert_index(unsigned int (&X)[N], int nb) {
    const unsigned int M = 1u << (nb - 1);
    for (unsigned int Q = M; Q > 1; Q >>= 1) {   // inverse undo
        const unsigned int P = Q - 1;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            if (X[i] & Q) X[0] ^= P;
            else { const unsigned int t = (X[0] ^ X[i]) & P; X[0] ^= t; X[i] ^= t; }
        }
    }
#pragma unroll
    for (int i = 1; i < N; ++i) X[i] ^= X[i - 1];   // Gray encode
    unsigned int t = 0;
    for (unsigned int Q = M; Q > 1; Q >>= 1)
        if (X[N - 1] & Q) t ^= Q - 1;
    unsigned long long key = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const unsigned long long x = X[i] ^ t;
        for (int b = 0; b < nb; ++b) key |= ((x >> b) & 1ull) << (N * b + (N - 1 - i));
    }
    return key;
}

// 3-D Hilbert index of the low nb bits of the cell coordinates (x, y, z)
__host__ __device__ static inline unsigned long long hilbert3_of_cell(unsigned int cx, unsigned int cy, unsigned int cz, int nb) {
    const unsigned int m = (1u << nb) - 1u;
    unsigned int X[3] = {cx & m, cy & m, cz & m};
    return hilbert_index<3>(X, nb);
}

// 2-D Hilbert index of the low nb bits of the cell coordinates (a, b), above the low nb_minor bits of the third coordinate
__host__ __device__ static inline unsigned long long hilbert2_minor_of_cell(unsigned int ca, unsigned int cb, unsigned int cminor, int nb, int nb_minor) {
    const unsigned int m = (1u << nb) - 1u;
    unsigned int X[2] = {ca & m, cb & m};
    return (hilbert_index<2>(X, nb) << nb_minor) | (unsigned long long)(cminor & ((1u << nb_minor) - 1u));
}

__device__ static inline unsigned long long hilbert3_key(double x, double y, double z, double lox, double loy, double loz, double inv, int nb) {
    bool clamped = false;
    const unsigned int cx = (unsigned int)cell_coord(x, lox, inv, &clamped);
    const unsigned int cy = (unsigned int)cell_coord(y, loy, inv, &clamped);
    const unsigned int cz = (unsigned int)cell_coord(z, loz, inv, &clamped);
    return hilbert3_of_cell(cx, cy, cz, nb);
}

__device__ static inline unsigned long long hilbert2_minor_key(double x, double y, double z, double lox, double loy, double loz, double inv,
                                                               const pcr_curve& cv) {
    bool clamped = false;
    const unsigned int c[3] = {(unsigned int)cell_coord(x, lox, inv, &clamped), (unsigned int)cell_coord(y, loy, inv, &clamped),
                               (unsigned int)cell_coord(z, loz, inv, &clamped)};
    // (selects, not a dynamically indexed array: the three coordinates stay in registers)
    const unsigned int ca = cv.ax[0] == 0 ? c[0] : cv.ax[0] == 1 ? c[1] : c[2];
    const unsigned int cb = cv.ax[1] == 0 ? c[0] : cv.ax[1] == 1 ? c[1] : c[2];
    const unsigned int cm = cv.ax[2] == 0 ? c[0] : cv.ax[2] == 1 ? c[1] : c[2];
    return hilbert2_minor_of_cell(ca, cb, cm, cv.nb, cv.nb_minor);
}

// The curve of a cloud with box [lo, hi] at 1 / cell `inv`, whose Morton key varies `end_bit` bits: the axes by falling extent
// (equal extents: the lower axis first); 2-D over the two longest with the third as minor key when the shortest extent is at most
// a quarter of the middle one (a scan is a surface: 3 m against 117 m on a KITTI frame), else 3-D.
static inline pcr_curve pcr_curve_pick(const double lo[3], const double hi[3], double inv, int end_bit, bool morton) {
    pcr_curve cv = {PCR_CURVE_MORTON, end_bit / 3, {0, 1, 2}, 0, end_bit};
    if (morton) return cv;
    const double e[3] = {hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]};
    for (int i = 1; i < 3; ++i)   // stable insertion sort, falling extent
        for (int j = i; j > 0 && e[cv.ax[j]] > e[cv.ax[j - 1]]; --j) { const int t = cv.ax[j]; cv.ax[j] = cv.ax[j - 1]; cv.ax[j - 1] = t; }
    if (e[cv.ax[2]] <= 0.25 * e[cv.ax[1]]) {
        const double kmax = floor(e[cv.ax[2]] * inv) + 2.0;   // as pcr_morton_end_bit counts an axis' bits
        int nbm = 1;
        while (nbm < cv.nb && (double)(1ll << nbm) <= kmax) ++nbm;
        cv.mode = PCR_CURVE_HILBERT2_MINOR;
        cv.nb_minor = nbm;
        cv.bits = 2 * cv.nb + nbm;
    } else {
        cv.mode = PCR_CURVE_HILBERT3;
        cv.bits = 3 * cv.nb;
    }
    return cv;
}
