// The one-sided Jacobi method on a 3 x 3 matrix and the frames taken from it, once: ransac.hip splits its essential matrix with
// it, ransac_h.hip decomposes its homography.  include/coponerf_hip.h (round 20) states the sequence, tests/ransac_ref.py restates
// it (split); float64, one rounding per operation, sums left to right as the parentheses say - the units that include this are
// built with -ffp-contract=off.  Matrices are row-major 9 doubles.
#pragma once
#include "common.h"

#include <math.h>

namespace {

constexpr int JACOBI_SWEEPS = 8;

// one rotation of the one-sided Jacobi method: columns p and q of G (and of V) are turned so that G's become orthogonal
__device__ __forceinline__ void jacobi_pair(double (&G)[9], double (&V)[9], int p, int q) {
    const double alpha = (G[p] * G[p] + G[3 + p] * G[3 + p]) + G[6 + p] * G[6 + p];
    const double beta = (G[q] * G[q] + G[3 + q] * G[3 + q]) + G[6 + q] * G[6 + q];
    const double gamma = (G[p] * G[q] + G[3 + p] * G[3 + q]) + G[6 + p] * G[6 + q];
    if (gamma == 0.0) return;
    const double zeta = (beta - alpha) / (2.0 * gamma);
    const double root = fabs(zeta) + sqrt(1.0 + zeta * zeta);
    const double tt = (zeta < 0.0 ? -1.0 : 1.0) / root;
    const double c = 1.0 / sqrt(1.0 + tt * tt), s = c * tt;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double gp = G[3 * r + p], gq = G[3 * r + q];
        G[3 * r + p] = c * gp - s * gq;
        G[3 * r + q] = s * gp + c * gq;
        const double vp = V[3 * r + p], vq = V[3 * r + q];
        V[3 * r + p] = c * vp - s * vq;
        V[3 * r + q] = s * vp + c * vq;
    }
}
__device__ __forceinline__ double norm3(const double* v) { return sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]); }
__device__ __forceinline__ void cross3(const double* a, const double* b, double* o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ void swap_columns(double (&G)[9], double (&V)[9], double (&sg)[3], int p, int q) {
    for (int r = 0; r < 3; ++r) {
        const double g = G[3 * r + p], v = V[3 * r + p];
        G[3 * r + p] = G[3 * r + q];
        G[3 * r + q] = g;
        V[3 * r + p] = V[3 * r + q];
        V[3 * r + q] = v;
    }
    const double x = sg[p];
    sg[p] = sg[q];
    sg[q] = x;
}
// G = M V with orthogonal columns after JACOBI_SWEEPS sweeps of the pairs (0, 1), (0, 2), (1, 2) from G = M, V = 1; the columns
// by descending norm sg (three compare-and-swaps, a swap only where strictly smaller comes first)
__device__ __forceinline__ void jacobi_svd(double (&G)[9], double (&V)[9], double (&sg)[3]) {
    for (int c = 0; c < 9; ++c) V[c] = (c % 4 == 0) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) {
        jacobi_pair(G, V, 0, 1);
        jacobi_pair(G, V, 0, 2);
        jacobi_pair(G, V, 1, 2);
    }
    for (int c = 0; c < 3; ++c) sg[c] = sqrt((G[c] * G[c] + G[3 + c] * G[3 + c]) + G[6 + c] * G[6 + c]);
    if (sg[0] < sg[1]) swap_columns(G, V, sg, 0, 1);
    if (sg[1] < sg[2]) swap_columns(G, V, sg, 1, 2);
    if (sg[0] < sg[1]) swap_columns(G, V, sg, 0, 1);
}
// a right-handed orthonormal frame from columns c0 and c1 of M: f0 = c0 / |c0|, f1 = (c1 - (f0 . c1) f0) / |..|, f2 = f0 x f1
__device__ __forceinline__ void frame(const double (&M)[9], int c0, int c1, double (&F)[3][3]) {
    const double a[3] = {M[c0], M[3 + c0], M[6 + c0]}, b[3] = {M[c1], M[3 + c1], M[6 + c1]};
    const double la = norm3(a);
    for (int i = 0; i < 3; ++i) F[0][i] = a[i] / la;
    const double d = (F[0][0] * b[0] + F[0][1] * b[1]) + F[0][2] * b[2];
    double w[3];
    for (int i = 0; i < 3; ++i) w[i] = b[i] - d * F[0][i];
    const double lw = norm3(w);
    for (int i = 0; i < 3; ++i) F[1][i] = w[i] / lw;
    cross3(F[0], F[1], F[2]);
}

}  // namespace
