// The linear system of a^T E b = 0 over R drawn matches and its null space, once: ransac.hip solves it with R = 8 (one null
// vector, which is E), ransac5.hip with R = 5 (four, which span E); ransac_h.hip fills the 8 x 9 system of a ~ H b instead
// (fill_rows_h) and takes the same elimination and null vector, which is H.  include/coponerf_hip.h (round 20) states the sequence,
// tests/ransac_ref.py restates it (eliminate, back_substitute); float64, one rounding per operation - the units that include this
// are built with -ffp-contract=off.
//
// A system is R x 9 doubles of the lane's column of an LDS array of L lanes, entry 9 r + c of lane l at A[9 r + c][l], where A
// points at the array's row that holds entry 0; perm[c][l] is the column of E at the permuted position c.  A lane touches its own
// column only - no barrier -, and a runtime index (the pivot's) never meets a private array.
#pragma once
#include "pinhole.h"
#include "ransac_common.h"
#include "sampson.h"

#include <math.h>

namespace epipolar_system {

constexpr double RANK_TOL = 1e-9;                          // round 20's: a pivot counts above RANK_TOL times the first

// the rows (a0 b0, a0 b1, a0, a1 b0, a1 b1, a1, b0, b1, 1) of the matches s[0 .. R) of the pair's `rows` -> all of them finite.
// It leaves at the first row that is not: a flag carried through all rows makes one long block instead, in which the compiler
// chains the 4 R divisions one behind the other (measured: the 8-point kernel 6 % slower).
template <int R, int L>
__device__ __forceinline__ bool fill_rows(double (*A)[L], int l, const float* __restrict__ rows, const int (&s)[R], const Cam& k0,
                                          const Cam& k1) {
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const float* const m = rows + (size_t)s[j] * 4;
        const float x0 = m[0], y0 = m[1], x1 = m[2], y1 = m[3];
        if (!(finite32(x0) && finite32(y0) && finite32(x1) && finite32(y1))) return false;
        const double a0 = ((double)x0 - k0.cx) / k0.fx, a1 = ((double)y0 - k0.cy) / k0.fy;
        const double b0 = ((double)x1 - k1.cx) / k1.fx, b1 = ((double)y1 - k1.cy) / k1.fy;
        A[9 * j + 0][l] = a0 * b0;
        A[9 * j + 1][l] = a0 * b1;
        A[9 * j + 2][l] = a0;
        A[9 * j + 3][l] = a1 * b0;
        A[9 * j + 4][l] = a1 * b1;
        A[9 * j + 5][l] = a1;
        A[9 * j + 6][l] = b0;
        A[9 * j + 7][l] = b1;
        A[9 * j + 8][l] = 1.0;
    }
    return true;
}

// the homography's system a ~ H b (ransac_h.hip, round 22): match j of s[0 .. R / 2) gives the rows 2 j = (b0, b1, 1, 0, 0, 0,
// -a0 b0, -a0 b1, -a0) and 2 j + 1 = (0, 0, 0, b0, b1, 1, -a1 b0, -a1 b1, -a1) -> all of them finite; p[j] takes (a0, a1, b0, b1)
template <int R, int L>
__device__ __forceinline__ bool fill_rows_h(double (*A)[L], int l, const float* __restrict__ rows, const int (&s)[R / 2], const Cam& k0,
                                            const Cam& k1, double (&p)[R / 2][4]) {
#pragma unroll
    for (int j = 0; j < R / 2; ++j) {
        const float* const m = rows + (size_t)s[j] * 4;
        const float x0 = m[0], y0 = m[1], x1 = m[2], y1 = m[3];
        if (!(finite32(x0) && finite32(y0) && finite32(x1) && finite32(y1))) return false;
        const double a0 = ((double)x0 - k0.cx) / k0.fx, a1 = ((double)y0 - k0.cy) / k0.fy;
        const double b0 = ((double)x1 - k1.cx) / k1.fx, b1 = ((double)y1 - k1.cy) / k1.fy;
        p[j][0] = a0, p[j][1] = a1, p[j][2] = b0, p[j][3] = b1;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double bc = c == 0 ? b0 : (c == 1 ? b1 : 1.0);
            A[18 * j + c][l] = bc;
            A[18 * j + 3 + c][l] = 0.0;
            A[18 * j + 6 + c][l] = -(a0 * bc);
            A[18 * j + 9 + c][l] = 0.0;
            A[18 * j + 12 + c][l] = bc;
            A[18 * j + 15 + c][l] = -(a1 * bc);
        }
    }
    return true;
}

// R steps of elimination with complete pivoting; false, and no further step, where a pivot is not finite or not above tol times
// the first one (the rank test)
template <int R, int L>
__device__ __forceinline__ bool eliminate(double (*A)[L], int (*perm)[L], int l, double tol) {
    for (int c = 0; c < 9; ++c) perm[c][l] = c;
    double p0 = 0.0;
    for (int k = 0; k < R; ++k) {
        double best = -1.0;
        int pr = k, pc = k;
        for (int r = k; r < R; ++r)
            for (int c = k; c < 9; ++c) {
                const double v = fabs(A[9 * r + c][l]);
                if (v > best) {                            // the first largest in (row, column) order; never a NaN
                    best = v;
                    pr = r;
                    pc = c;
                }
            }
        if (pr != k)
            for (int c = 0; c < 9; ++c) {
                const double v = A[9 * k + c][l];
                A[9 * k + c][l] = A[9 * pr + c][l];
                A[9 * pr + c][l] = v;
            }
        if (pc != k) {
            for (int r = 0; r < R; ++r) {
                const double v = A[9 * r + k][l];
                A[9 * r + k][l] = A[9 * r + pc][l];
                A[9 * r + pc][l] = v;
            }
            const int v = perm[k][l];
            perm[k][l] = perm[pc][l];
            perm[pc][l] = v;
        }
        const double p = A[9 * k + k][l];
        if (k == 0) p0 = fabs(p);
        if (!(finite64(p) && fabs(p) > tol * p0)) return false;
        for (int r = k + 1; r < R; ++r) {
            const double m = A[9 * r + k][l] / p;
            for (int c = k + 1; c < 9; ++c) A[9 * r + c][l] = A[9 * r + c][l] - m * A[9 * k + c][l];
        }
    }
    return true;
}

// null vector v of the eliminated system: the free unknown R + v is 1, the other free ones 0, back substitution into X (9 entries
// in the permuted order), then entry perm[c] of dst takes X[c].  dst may be A itself once the system is spent.
template <int R, int L>
__device__ __forceinline__ void null_vector(const double (*A)[L], double (*X)[L], const int (*perm)[L], int l, int v,
                                            double (*dst)[L]) {
    for (int c = R; c < 9; ++c) X[c][l] = c == R + v ? 1.0 : 0.0;
    for (int r = R - 1; r >= 0; --r) {
        double sum = A[9 * r + r + 1][l] * X[r + 1][l];
        for (int c = r + 2; c < 9; ++c) sum = sum + A[9 * r + c][l] * X[c][l];
        X[r][l] = -sum / A[9 * r + r][l];
    }
    for (int c = 0; c < 9; ++c) dst[perm[c][l]][l] = X[c][l];
}

// e / |e|_F with the first largest |e_c| positive -> every entry finite
__device__ __forceinline__ bool unit_essential(double (&e)[9]) {
    double ss = e[0] * e[0];
#pragma unroll
    for (int c = 1; c < 9; ++c) ss = ss + e[c] * e[c];
    const double nrm = sqrt(ss);
    double big = -1.0, lead = 0.0;
#pragma unroll
    for (int c = 0; c < 9; ++c) {
        e[c] = e[c] / nrm;
        if (fabs(e[c]) > big) {
            big = fabs(e[c]);
            lead = e[c];
        }
    }
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 9; ++c) {
        if (lead < 0.0) e[c] = -e[c];
        ok = ok && finite64(e[c]);
    }
    return ok;
}

}  // namespace epipolar_system
