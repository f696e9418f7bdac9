// Small dense routines of the spectral solver, one source for the host (pcr_sym_eig_jacobi, the dense path of small clouds) and the
// device (the Rayleigh-Ritz step in the last block of the Gram kernel), like pcr_gmm_log_density.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

// Cyclic Jacobi eigen-solve of the symmetric n x n matrix A (row-major; both triangles are read and kept equal).  On return the
// diagonal of A holds the eigenvalues (unsorted) and column j of V (row-major n x n) the unit eigenvector of A[j][j].
// `nl` lanes share the work: lane `lane` updates the rows k = lane, lane + nl, ...; sync() orders their accesses to A and V (the
// host calls it with one lane and an empty sync).  Every lane takes the same decisions from the same memory, every entry is computed
// by exactly one lane with the same expression: the result does not depend on nl.
// A rotation is skipped where |a_pq| <= 1e-18 |A|_F; a sweep without rotations ends the solve (at most 64 sweeps).
template <class Sync>
__host__ __device__ static inline void pcr_jacobi_eig(int n, double* A, double* V, int lane, int nl, Sync sync) {
    for (int i = lane; i < n * n; i += nl) V[i] = (i / n == i % n) ? 1.0 : 0.0;
    double nrm = 0.0;
    for (int i = 0; i < n * n; ++i) nrm += A[i] * A[i];
    const double thr = sqrt(nrm) * 1e-18;
    sync();
    for (int sweep = 0; sweep < 64; ++sweep) {
        int rotated = 0;
        for (int p = 0; p < n - 1; ++p) {
            for (int q = p + 1; q < n; ++q) {
                const double apq = A[p * n + q];
                if (!(fabs(apq) > thr)) continue;
                ++rotated;
                const double app = A[p * n + p], aqq = A[q * n + q];
                const double theta = (aqq - app) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                sync();   // every lane has read a_pq, a_pp, a_qq
                for (int k = lane; k < n; k += nl) {
                    if (k == p) {
                        A[p * n + p] = app - t * apq;
                        A[q * n + q] = aqq + t * apq;
                        A[p * n + q] = 0.0;
                        A[q * n + p] = 0.0;
                    } else if (k != q) {
                        const double akp = A[k * n + p], akq = A[k * n + q];
                        const double r = c * akp - s * akq, u = s * akp + c * akq;
                        A[k * n + p] = r; A[p * n + k] = r;
                        A[k * n + q] = u; A[q * n + k] = u;
                    }
                    const double vkp = V[k * n + p], vkq = V[k * n + q];
                    V[k * n + p] = c * vkp - s * vkq;
                    V[k * n + q] = s * vkp + c * vkq;
                }
                sync();
            }
        }
        if (!rotated) break;
    }
}

// order[0 .. n): the indices of diag(A) in descending order of the value, the lower index first among equals
__host__ __device__ static inline void pcr_order_desc(int n, const double* A, int* order) {
    for (int i = 0; i < n; ++i) order[i] = i;
    for (int i = 1; i < n; ++i) {   // insertion sort, stable
        const int o = order[i];
        int j = i;
        while (j > 0 && A[order[j - 1] * n + order[j - 1]] < A[o * n + o]) { order[j] = order[j - 1]; --j; }
        order[j] = o;
    }
}

// start vector of the block iteration: a hash of (caller row, column) to (-1, 1), no RNG state (splitmix64's finaliser)
__host__ __device__ static inline double pcr_spectral_start(long long row, int col) {
    unsigned long long z = ((unsigned long long)row * 16ull + (unsigned long long)col) * 0x9e3779b97f4a7c15ull + 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    z = z ^ (z >> 31);
    return (double)(2ull * (z >> 12) + 1ull) * (1.0 / 4503599627370496.0) - 1.0;   // (2 j + 1) 2^-52 - 1, j < 2^52: exact, never -1, 0 or 1
}
