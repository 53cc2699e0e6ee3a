// The minimal solver of coponerf_amd/matches.py: ransac_pose(solver="5pt"): up to 10 essential matrices from 5 matches.
//
//   ransac_hypotheses5_kernel  cpn_ransac_hypotheses5: one thread per sample index h (workgroups of 32), every pair in the launch.
//                              The thread draws 5 distinct rows (ransac_common.h: the first 5 of round 20's 8), eliminates the
//                              5 x 9 system with complete pivoting and takes the four null vectors by back substitution
//                              (epipolar_system.h: the 8-point solver's code with 5 rows, its norm and sign too), forms the
//                              ten cubic constraints on E = x X + y Y + z Z + W as a 10 x 20 matrix, reduces it by Gauss-Jordan
//                              elimination, and finds the real roots of the degree-10 determinant in z by a Sturm chain,
//                              bisection and Newton steps.  cpn_ransac_score and cpn_ransac_finish (ransac.hip) take the 10 Hn
//                              slots as they take any hypotheses.
//
// Layout.  Everything a runtime index reaches - the systems, the permutation, the Sturm chain - lives in LDS as [entry][lane]
// (a lane's accesses never meet another lane's bank, and no lane reads another's column: no barrier); everything else is a
// private array whose indices are constants once its loops are unrolled, i.e. registers.  The 10 x 20 matrix, the four null
// vectors behind it and the 5 x 9 system that it overwrites are 236 doubles per lane: 59 KiB for 32 lanes, which any two
// workgroups of a CU hold side by side; 64 lanes would be 118 KiB, one workgroup per CU, for nothing - 1024 samples are 32
// workgroups of 32 against 256 CUs either way.
//
// Every operation is one of + - * / sqrt or a comparison, with one rounding (-ffp-contract=off) and fixed trip counts, in the
// sequence of tests/ransac5_ref.py: the kernel's bits are the restatement's.
#include "common.h"
#include "epipolar_system.h"
#include "pinhole.h"
#include "ransac_common.h"
#include "sampson.h"

#include "../../include/coponerf_hip.h"

#include <math.h>

namespace {

namespace es = epipolar_system;
constexpr int L5 = 32;                                     // samples (lanes) per workgroup
constexpr double RANK_TOL10 = 1e-10;                       // the 10 x 20 elimination; the 5 x 9 one keeps round 20's
constexpr int BISECT = 40;
constexpr int NEWTON = 4;
// LDS entries per lane
constexpr int S_A = 0;                                     // the 5 x 9 system, entry 9 r + c
constexpr int S_X = 45;                                    // a back substitution's unknowns in the permuted order
constexpr int S_M = 0;                                     // the 10 x 20 matrix, entry 20 r + c (the system is spent)
constexpr int S_F = 0;                                     // the Sturm chain, f_i at S_F + chain_at(i) (the matrix is spent)
constexpr int S_R = 66;                                    // a remainder at work, 11 entries
constexpr int S_P1 = 80, S_P2 = 88, S_P3 = 96;             // the cross product of rows 0 and 1 of B(z): 8, 8 and 7 coefficients
constexpr int S_N = 200;                                   // the four null vectors, entry 9 v + c
constexpr int S_ALL = 236;

// ---- the monomials: variables 0 = x, 1 = y, 2 = z, 3 = 1; pairs and triples in lexicographic order
__device__ __forceinline__ constexpr int pair_at(int i, int j) {                 // i <= j
    return 4 * i - i * (i - 1) / 2 + (j - i);
}
__device__ __forceinline__ constexpr int min2(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ constexpr int max2(int a, int b) { return a > b ? a : b; }
// the column of the monomial v_i v_j v_k in the header's order
//   x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1
__device__ __forceinline__ constexpr int column_of(int i, int j, int k) {
    const int lo = min2(i, min2(j, k)), hi = max2(i, max2(j, k)), mid = i + j + k - lo - hi;
    switch (16 * lo + 4 * mid + hi) {
        case 0: return 0;                                  // 000 x^3
        case 21: return 1;                                 // 111 y^3
        case 1: return 2;                                  // 001 x^2 y
        case 5: return 3;                                  // 011 x y^2
        case 2: return 4;                                  // 002 x^2 z
        case 3: return 5;                                  // 003 x^2
        case 22: return 6;                                 // 112 y^2 z
        case 23: return 7;                                 // 113 y^2
        case 6: return 8;                                  // 012 x y z
        case 7: return 9;                                  // 013 x y
        case 10: return 10;                                // 022 x z^2
        case 11: return 11;                                // 023 x z
        case 15: return 12;                                // 033 x
        case 26: return 13;                                // 122 y z^2
        case 27: return 14;                                // 123 y z
        case 31: return 15;                                // 133 y
        case 42: return 16;                                // 222 z^3
        case 43: return 17;                                // 223 z^2
        case 47: return 18;                                // 233 z
        default: return 19;                                // 333 1
    }
}
constexpr int PAIR_I[10] = {0, 0, 0, 0, 1, 1, 1, 2, 2, 3}, PAIR_J[10] = {0, 1, 2, 3, 1, 2, 3, 2, 3, 3};

// two linear forms -> the quadratic: o[pair(i, j)] += a_i b_j, i outer, j inner, from 0
__device__ __forceinline__ void mul11(const double (&a)[4], const double (&b)[4], double (&o)[10]) {
#pragma unroll
    for (int m = 0; m < 10; ++m) o[m] = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int q = pair_at(min2(i, j), max2(i, j));
            o[q] = o[q] + a[i] * b[j];
        }
}
// a quadratic times a linear form -> the cubic in the header's column order: o[column] += a_m b_k, m outer, k inner, from 0
__device__ __forceinline__ void mul21(const double (&a)[10], const double (&b)[4], double (&o)[20]) {
#pragma unroll
    for (int c = 0; c < 20; ++c) o[c] = 0.0;
#pragma unroll
    for (int m = 0; m < 10; ++m)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = column_of(PAIR_I[m], PAIR_J[m], k);
            o[c] = o[c] + a[m] * b[k];
        }
}
// (p0 t0 - p1 t1) + p2 t2 with sign = -1, (p0 t0 + p1 t1) + p2 t2 with sign = +1, into row `row` of the matrix
template <int SIGN>
__device__ __forceinline__ void cubic_row(double (*S)[L5], int l, int row, const double (&p0)[10], const double (&t0)[4],
                                          const double (&p1)[10], const double (&t1)[4], const double (&p2)[10],
                                          const double (&t2)[4]) {
    double u[20], v[20], w[20];
    mul21(p0, t0, u);
    mul21(p1, t1, v);
    mul21(p2, t2, w);
#pragma unroll
    for (int c = 0; c < 20; ++c) S[S_M + 20 * row + c][l] = (SIGN < 0 ? u[c] - v[c] : u[c] + v[c]) + w[c];
}
// polynomials in z, ascending: o[i + j] += a_i b_j, i outer, j inner, from 0
template <int NA, int NB>
__device__ __forceinline__ void conv(const double (&a)[NA], const double (&b)[NB], double (&o)[NA + NB - 1]) {
#pragma unroll
    for (int k = 0; k < NA + NB - 1; ++k) o[k] = 0.0;
#pragma unroll
    for (int i = 0; i < NA; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) o[i + j] = o[i + j] + a[i] * b[j];
}
template <int NA, int NB>
__device__ __forceinline__ void conv_diff(const double (&a)[NA], const double (&b)[NB], const double (&c)[NA], const double (&d)[NB],
                                          double (&o)[NA + NB - 1]) {                 // a b - c d
    double u[NA + NB - 1], v[NA + NB - 1];
    conv(a, b, u);
    conv(c, d, v);
#pragma unroll
    for (int k = 0; k < NA + NB - 1; ++k) o[k] = u[k] - v[k];
}

__device__ __forceinline__ constexpr int chain_at(int i) { return 11 * i - i * (i - 1) / 2; }      // f_i has 11 - i coefficients
// the polynomial of n coefficients at entry `at` of the lane's LDS column, by Horner's rule
__device__ __forceinline__ double horner(const double (*S)[L5], int l, int at, int n, double z) {
    double v = S[at + n - 1][l];
    for (int k = n - 2; k >= 0; --k) v = v * z + S[at + k][l];
    return v;
}
__device__ __forceinline__ void count_sign(double v, int& last, int& changes) {
    const int s = (v > 0.0 ? 1 : 0) - (v < 0.0 ? 1 : 0);
    if (s != 0) {
        if (last != 0 && s != last) ++changes;
        last = s;
    }
}
// the sign changes of f_0 .. f_10 at z, zeros skipped
__device__ __forceinline__ int sturm_changes(const double (*S)[L5], int l, double z) {
    int changes = 0, last = 0;
    for (int i = 0; i < 11; ++i) count_sign(horner(S, l, S_F + chain_at(i), 11 - i, z), last, changes);
    return changes;
}
__device__ __forceinline__ double line_of(double t) { return t / (1.0 - fabs(t)); }             // (-1, 1) onto the real line

__global__ __launch_bounds__(L5) void ransac_hypotheses5_kernel(const float* __restrict__ xy, const int* __restrict__ count,
                                                                const float* __restrict__ intrinsics, int N, int Hn,
                                                                unsigned long long seed, double* __restrict__ E,
                                                                int* __restrict__ sample, uint8_t* __restrict__ valid) {
    __shared__ double S[S_ALL][L5];
    __shared__ int perm[9][L5];                            // the column of E at each permuted position
    const int l = threadIdx.x, h = blockIdx.x * L5 + l, b = blockIdx.y;
    if (h >= Hn) return;                                   // no barrier below: a lane touches its own LDS column only
    const int n = clamp_count(count[b], N);
    const size_t at = (size_t)b * Hn + h;

    // ---- the draw
    int s[5];
    const int got = ransac_draw::draw_rows<5>(seed, h, n, s);
#pragma unroll
    for (int j = 0; j < 5; ++j) sample[at * 5 + j] = s[j];

    // ---- the system, 5 steps of elimination, and the four null vectors: the free unknown 5 + v is 1, the other three 0
    bool ok = got == 5;
    if (ok) {
        const Cam k0 = load_cam(intrinsics + ((size_t)b * 2 + 0) * 16), k1 = load_cam(intrinsics + ((size_t)b * 2 + 1) * 16);
        ok = es::fill_rows<5>(S + S_A, l, xy + (size_t)b * N * 4, s, k0, k1);
    }
    if (ok) ok = es::eliminate<5>(S + S_A, perm, l, es::RANK_TOL);
    if (ok)
        for (int v = 0; v < 4; ++v) es::null_vector<5>(S + S_A, S + S_X, perm, l, v, S + S_N + 9 * v);
    // ---- the ten cubic constraints on E = x X + y Y + z Z + W
    if (ok) {
        double e[9][4];                                    // entry c of E as a linear form in (x, y, z, 1)
#pragma unroll
        for (int c = 0; c < 9; ++c)
#pragma unroll
            for (int v = 0; v < 4; ++v) e[c][v] = S[S_N + 9 * v + c][l];
        {                                                  // row 0: det E = (q0 e0 - q1 e1) + q2 e2
            double q0[10], q1[10], q2[10], u[10], w[10];
            mul11(e[4], e[8], u);
            mul11(e[5], e[7], w);
#pragma unroll
            for (int m = 0; m < 10; ++m) q0[m] = u[m] - w[m];
            mul11(e[3], e[8], u);
            mul11(e[5], e[6], w);
#pragma unroll
            for (int m = 0; m < 10; ++m) q1[m] = u[m] - w[m];
            mul11(e[3], e[7], u);
            mul11(e[4], e[6], w);
#pragma unroll
            for (int m = 0; m < 10; ++m) q2[m] = u[m] - w[m];
            cubic_row<-1>(S, l, 0, q0, e[0], q1, e[1], q2, e[2]);
        }
        double G[3][3][10];                                // E E^T - tr(E E^T) / 2, the symmetric half filled twice
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = i; j < 3; ++j) {
                double u[10], v[10], w[10];
                mul11(e[3 * i], e[3 * j], u);
                mul11(e[3 * i + 1], e[3 * j + 1], v);
                mul11(e[3 * i + 2], e[3 * j + 2], w);
#pragma unroll
                for (int m = 0; m < 10; ++m) G[i][j][m] = G[j][i][m] = (u[m] + v[m]) + w[m];
            }
#pragma unroll
        for (int m = 0; m < 10; ++m) {
            const double half = 0.5 * ((G[0][0][m] + G[1][1][m]) + G[2][2][m]);
            G[0][0][m] = G[0][0][m] - half;
            G[1][1][m] = G[1][1][m] - half;
            G[2][2][m] = G[2][2][m] - half;
        }
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) cubic_row<1>(S, l, 1 + 3 * i + j, G[i][0], e[j], G[i][1], e[3 + j], G[i][2], e[6 + j]);
    }
    // ---- Gauss-Jordan elimination with partial pivoting; rows 0 .. 3 are not reduced upwards: nothing reads them
    if (ok) {
        double p0 = 0.0;
        for (int k = 0; k < 10; ++k) {
            double best = -1.0;
            int pr = k;
            for (int r = k; r < 10; ++r) {
                const double v = fabs(S[S_M + 20 * r + k][l]);
                if (v > best) {
                    best = v;
                    pr = r;
                }
            }
            if (pr != k)
                for (int c = k; c < 20; ++c) {
                    const double v = S[S_M + 20 * k + c][l];
                    S[S_M + 20 * k + c][l] = S[S_M + 20 * pr + c][l];
                    S[S_M + 20 * pr + c][l] = v;
                }
            const double p = S[S_M + 20 * k + k][l];
            if (k == 0) p0 = fabs(p);
            ok = finite64(p) && fabs(p) > RANK_TOL10 * p0; // the rank test
            if (!ok) break;
            for (int c = k + 1; c < 20; ++c) S[S_M + 20 * k + c][l] = S[S_M + 20 * k + c][l] / p;
            for (int r = 0; r < 10; ++r)
                if (r > k || (r >= 4 && r < k)) {
                    const double m = S[S_M + 20 * r + k][l];
                    for (int c = k + 1; c < 20; ++c) S[S_M + 20 * r + c][l] = S[S_M + 20 * r + c][l] - m * S[S_M + 20 * k + c][l];
                }
        }
    }
    // ---- B(z), its determinant and the Sturm chain
    int roots = 0, changes_left = 0;
    if (ok) {
        double Bx[3][4], By[3][4], Bc[3][5];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            double a[10], c[10];                           // columns 10 .. 19 of rows 4 + 2 i and 5 + 2 i
#pragma unroll
            for (int k = 0; k < 10; ++k) {
                a[k] = S[S_M + 20 * (4 + 2 * i) + 10 + k][l];
                c[k] = S[S_M + 20 * (5 + 2 * i) + 10 + k][l];
            }
            Bx[i][0] = a[2], Bx[i][1] = a[1] - c[2], Bx[i][2] = a[0] - c[1], Bx[i][3] = -c[0];
            By[i][0] = a[5], By[i][1] = a[4] - c[5], By[i][2] = a[3] - c[4], By[i][3] = -c[3];
            Bc[i][0] = a[9], Bc[i][1] = a[8] - c[9], Bc[i][2] = a[7] - c[8], Bc[i][3] = a[6] - c[7], Bc[i][4] = -c[6];
        }
        double p1[8], p2[8], p3[7], det[11];
        conv_diff(By[0], Bc[1], By[1], Bc[0], p1);         // B01 B12 - B11 B02
        conv_diff(Bx[1], Bc[0], Bx[0], Bc[1], p2);         // B10 B02 - B00 B12
        conv_diff(Bx[0], By[1], Bx[1], By[0], p3);         // B00 B11 - B10 B01
        {
            double u[11], v[11], w[11];
            conv(p1, Bx[2], u);
            conv(p2, By[2], v);
            conv(p3, Bc[2], w);
#pragma unroll
            for (int k = 0; k < 11; ++k) det[k] = (u[k] + v[k]) + w[k];
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            S[S_P1 + k][l] = p1[k];
            S[S_P2 + k][l] = p2[k];
        }
#pragma unroll
        for (int k = 0; k < 7; ++k) S[S_P3 + k][l] = p3[k];
        // f_0 = det / |det_10|, f_1 = f_0', f_(i + 1) = -rem(f_(i - 1), f_i) / |its leading coefficient|
        const double lead = fabs(det[10]);
        ok = finite64(lead) && lead > 0.0;
#pragma unroll
        for (int k = 0; k < 11; ++k) S[S_F + k][l] = det[k] / lead;
        for (int k = 1; k < 11; ++k) S[S_F + 11 + k - 1][l] = (double)k * S[S_F + k][l];
        for (int i = 1; i < 10; ++i) {
            const int deg = 11 - i, prev = S_F + chain_at(i - 1), cur = S_F + chain_at(i), next = S_F + chain_at(i + 1);
            for (int k = 0; k <= deg; ++k) S[S_R + k][l] = S[prev + k][l];
            const double g = S[cur + deg - 1][l];
            double q = S[S_R + deg][l] / g;
            for (int k = 0; k < deg - 1; ++k) S[S_R + k + 1][l] = S[S_R + k + 1][l] - q * S[cur + k][l];
            q = S[S_R + deg - 1][l] / g;
            for (int k = 0; k < deg - 1; ++k) S[S_R + k][l] = S[S_R + k][l] - q * S[cur + k][l];
            const double top = fabs(S[S_R + deg - 2][l]);
            ok = ok && finite64(top) && top > 0.0;
            for (int k = 0; k < deg - 1; ++k) S[next + k][l] = -(S[S_R + k][l] / top);
        }
        // the sign changes at -inf and +inf: those of the leading coefficients, times (-1)^degree at -inf
        int last_l = 0, last_r = 0, changes_right = 0;
        for (int i = 0; i < 11; ++i) {
            const double c = S[S_F + chain_at(i) + 10 - i][l];
            count_sign((i & 1) ? -c : c, last_l, changes_left);
            count_sign(c, last_r, changes_right);
        }
        roots = changes_left - changes_right;
        roots = roots < 0 ? 0 : (roots > 10 ? 10 : roots);
    }
    // ---- the roots in ascending order, and E at each
    for (int r = 0; r < 10; ++r) {
        double e[9];
#pragma unroll
        for (int c = 0; c < 9; ++c) e[c] = 0.0;
        bool on = ok && r < roots;
        if (on) {
            double lo = -1.0, hi = 1.0;
            for (int step = 0; step < BISECT; ++step) {
                const double mid = (lo + hi) * 0.5;
                if (changes_left - sturm_changes(S, l, line_of(mid)) >= r + 1)
                    hi = mid;
                else
                    lo = mid;
            }
            const double zlo = line_of(lo), zhi = line_of(hi);
            double z = line_of((lo + hi) * 0.5);
            for (int step = 0; step < NEWTON; ++step) {
                const double zn = z - horner(S, l, S_F, 11, z) / horner(S, l, S_F + 11, 10, z);
                if (zn >= zlo && zn <= zhi) z = zn;
            }
            const double d = horner(S, l, S_P3, 7, z);
            const double x = horner(S, l, S_P1, 8, z) / d, y = horner(S, l, S_P2, 8, z) / d;
#pragma unroll
            for (int c = 0; c < 9; ++c)
                e[c] = ((x * S[S_N + c][l] + y * S[S_N + 9 + c][l]) + z * S[S_N + 18 + c][l]) + S[S_N + 27 + c][l];
            on = es::unit_essential(e);
        }
#pragma unroll
        for (int c = 0; c < 9; ++c) E[(at * 10 + r) * 9 + c] = on ? e[c] : 0.0;
        valid[at * 10 + r] = on ? 1 : 0;
    }
}

}  // namespace

extern "C" int cpn_ransac_hypotheses5(const float* xy, const int* count, const float* intrinsics, int B, int N, int Hn, long long seed,
                                      double* E, int* sample, uint8_t* valid, void* stream) {
    CPN_REQUIRE(xy && count && intrinsics && E && sample && valid, CPN_E_ARG, "cpn_ransac_hypotheses5: null pointer");
    CPN_REQUIRE(shape_ok(B, N, 10LL * Hn) && Hn >= 1, CPN_E_SHAPE,
                "cpn_ransac_hypotheses5: need 1 <= B <= 32767, 1 <= N <= 2^24, 1 <= 10 Hn <= 2^20 and B chunks (10 Hn + 1) < 2^31 (got "
                "B %d, N %d, Hn %d)", B, N, Hn);
    hipLaunchKernelGGL(ransac_hypotheses5_kernel, dim3(cpn_cdiv(Hn, L5), B), dim3(L5), 0, (hipStream_t)stream, xy, count, intrinsics,
                       N, Hn, (unsigned long long)seed, E, sample, valid);
    CPN_LAUNCH_CHECK("cpn_ransac_hypotheses5");
    return 0;
}
