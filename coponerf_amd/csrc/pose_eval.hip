// How good is a pose, and how good are the matches under it (coponerf_amd/matches.py pose_errors / residual_stats, the columns
// Evaluator(geometry=...) writes): round 25 of include/coponerf_hip.h, which states the operation order.
//
//   pose_errors_kernel     cpn_pose_errors: one thread per (pair, pose): the rotation angle, the translation distance and the
//                          direction angle to the ground truth in float64, both angles by atan2 - well conditioned at 1e-6 degrees
//                          and at 179.9999, where fp32 acos is not.
//   residual_stats_kernel  cpn_residual_stats: grid (P, B), ONE workgroup of 256 threads per (pose, pair), cpn_refine_pose's shape.
//                          Exact order statistics of the usable |r| (sampson.h's residual under E = [t]x R of the pose) by a radix
//                          descent on the 64-bit pattern of |r|, 8 bits a pass: non-negative doubles order as their patterns.  The
//                          residual is recomputed in every pass from the same inputs - bit-identical, no scratch of B P N doubles -,
//                          the digit histograms are integer LDS adds (a count does not depend on the order of arrival).  Pass 0
//                          takes the top digit of every usable row, counts them and the rows within the thresholds; passes 1 .. 7
//                          one histogram per wanted rank over the rows that carry its prefix; a last pass sums r^2 below the
//                          2.5 sigma cut in pose_gauss_newton.h's block order.  Ten passes over the rows, no sort, no global
//                          atomics, nothing in HBM but the outputs.
//
// float64 from the fp32 inputs, one rounding per operation (-ffp-contract=off), sums left to right: tests/pose_eval_ref.py restates
// both kernels in numpy.  Cam and Pose are pinhole.h's; essential, sampson, residual_ok and finite64 sampson.h's; the count clamp
// ransac_common.h's; the descent radix_select.h's, which cpn_depth_scale (triangulate.hip) ranks with as well.
#include "common.h"
#include "pinhole.h"
#include "radix_select.h"
#include "ransac_common.h"
#include "sampson.h"

#include <math.h>

namespace {

constexpr int NT = 256;
constexpr int SLOTS = CPN_POSE_EVAL_MAX + 1;               // the wanted ranks: Q quantiles and the median of the sigmas

// the quantiles and thresholds travel as kernel arguments: the entry point has checked them on the host
struct StatArgs {
    double q[CPN_POSE_EVAL_MAX], thr[CPN_POSE_EVAL_MAX];
    int Q, T;
};

__device__ __forceinline__ double nan64() { return __builtin_nan(""); }

__device__ __forceinline__ double norm3(double x, double y, double z) { return sqrt((x * x + y * y) + z * z); }

__global__ __launch_bounds__(NT) void pose_errors_kernel(const float* __restrict__ poses, const float* __restrict__ gt, int B, int P,
                                                         double* __restrict__ out) {
    const int item = blockIdx.x * NT + threadIdx.x;
    if (item >= B * P) return;
    const Pose a = load_pose(poses + (size_t)item * 16), g = load_pose(gt + (size_t)(item / P) * 16);
    double* const o = out + (size_t)item * 3;
    if (!(pose_finite(a) && pose_finite(g))) {
        o[0] = o[1] = o[2] = nan64();
        return;
    }
    double M[3][3];                                        // M = R R_gt^T
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) M[i][j] = (a.R[i][0] * g.R[j][0] + a.R[i][1] * g.R[j][1]) + a.R[i][2] * g.R[j][2];
    const double s = 0.5 * norm3(M[2][1] - M[1][2], M[0][2] - M[2][0], M[1][0] - M[0][1]);
    const double c = (((M[0][0] + M[1][1]) + M[2][2]) - 1.0) / 2.0;
    o[0] = atan2(s, c);
    o[1] = norm3(a.t[0] - g.t[0], a.t[1] - g.t[1], a.t[2] - g.t[2]);
    const bool zero = (a.t[0] == 0.0 && a.t[1] == 0.0 && a.t[2] == 0.0) || (g.t[0] == 0.0 && g.t[1] == 0.0 && g.t[2] == 0.0);
    const double x = norm3(a.t[1] * g.t[2] - a.t[2] * g.t[1], a.t[2] * g.t[0] - a.t[0] * g.t[2], a.t[0] * g.t[1] - a.t[1] * g.t[0]);
    const double d = (a.t[0] * g.t[0] + a.t[1] * g.t[1]) + a.t[2] * g.t[2];
    o[2] = zero ? nan64() : atan2(x, d);
}

// |r| of row m under E, and whether the row is usable
__device__ __forceinline__ double abs_residual(const double (&E)[9], const Cam& k0, const Cam& k1, const float* __restrict__ m,
                                               bool& ok) {
    const Sampson s = sampson(E, k0, k1, (double)m[0], (double)m[1], (double)m[2], (double)m[3]);
    const double r = s.n / sqrt(s.D);
    ok = residual_ok(s, r);
    return fabs(r);                                        // -0 and +0 are one key
}

struct StatShared {
    radix::Select<SLOTS> sel;                              // radix_select.h: the histograms, the prefixes and the ranks
    int within[CPN_POSE_EVAL_MAX];
    double red[4];
    int n_in[4];
};

__global__ __launch_bounds__(NT) void residual_stats_kernel(const float* __restrict__ xy, const int* __restrict__ count,
                                                            const float* __restrict__ intrinsics, const float* __restrict__ poses,
                                                            const StatArgs args, int N, int* __restrict__ usable,
                                                            double* __restrict__ quant, int* __restrict__ within,
                                                            double* __restrict__ sigma, int* __restrict__ status) {
    __shared__ StatShared sh;
    const int p = blockIdx.x, b = blockIdx.y, P = gridDim.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int Q = args.Q, T = args.T, slots = Q + 1;
    const size_t item = (size_t)b * P + p;
    const int n = clamp_count(count[b], N);
    const float* const rows = xy + (size_t)b * N * 4;
    const Pose pose = load_pose(poses + item * 16);
    const bool pose_ok = pose_finite(pose) && !(pose.t[0] == 0.0 && pose.t[1] == 0.0 && pose.t[2] == 0.0);
    const Cam k0 = load_cam(intrinsics + ((size_t)b * 2 + 0) * 16), k1 = load_cam(intrinsics + ((size_t)b * 2 + 1) * 16);
    double E[9];
    essential(&pose.R[0][0], pose.t, E);
    // the value being ranked: |r| of the row, recomputed wherever it is asked for
    const auto value = [&](int i, double& r) {
        bool ok;
        r = abs_residual(E, k0, k1, rows + (size_t)i * 4, ok);
        return ok;
    };

    // ---- pass 0: the top digit of every usable row (their sum is n_u) and the rows within the thresholds
    if (tid < CPN_POSE_EVAL_MAX) sh.within[tid] = 0;
    int in[CPN_POSE_EVAL_MAX];
#pragma unroll
    for (int t = 0; t < CPN_POSE_EVAL_MAX; ++t) in[t] = 0;
    const int n_u = radix::top_digits<NT>(sh.sel, pose_ok ? n : 0, value, [&](double r) {
#pragma unroll
        for (int t = 0; t < CPN_POSE_EVAL_MAX; ++t) in[t] += (t < T && r <= args.thr[t]) ? 1 : 0;
    });
    if (n_u == 0) {                                        // nothing to rank: every element of the five outputs all the same
        if (tid == 0) {
            usable[item] = 0;
            status[item] = pose_ok ? 1 : 2;
            sigma[item * 2 + 0] = sigma[item * 2 + 1] = nan64();
        }
        if (tid < Q) quant[item * Q + tid] = nan64();
        if (tid < T) within[item * T + tid] = 0;
        return;
    }
#pragma unroll
    for (int t = 0; t < CPN_POSE_EVAL_MAX; ++t)
        if (t < T && in[t]) atomicAdd(&sh.within[t], in[t]);  // read behind the descent's barriers

    // ---- the wanted ranks, and the descent: slot j < Q is quantile j, slot Q the median
    radix::select<NT>(sh.sel, slots, n, value, [&](int j) {
        const long long k = j < Q ? (long long)floor(args.q[j] * (double)(n_u - 1)) : (long long)((n_u - 1) >> 1);
        return k < 0 ? 0 : (k > n_u - 1 ? (long long)(n_u - 1) : k);
    });

    // ---- the sigmas: Rousseeuw's LMedS scale with p = 5 from the median, then the rows within 2.5 of it
    const double med = __longlong_as_double((long long)sh.sel.prefix[Q]);
    const double s0 = n_u > 5 ? (1.4826 * (1.0 + 5.0 / (double)(n_u - 5))) * med : nan64();
    const double cut = 2.5 * s0;
    double acc = 0.0;
    int mine = 0;
    for (int i = tid; i < n; i += NT) {
        bool ok;
        const double r = abs_residual(E, k0, k1, rows + (size_t)i * 4, ok);
        if (ok && r <= cut) {                              // false for a NaN cut
            acc += r * r;
            ++mine;
        }
    }
    acc = wave_sum(acc);
    mine = wave_sum(mine);
    if (lane == 0) {
        sh.red[wave] = acc;
        sh.n_in[wave] = mine;
    }
    __syncthreads();
    if (tid == 0) {
        const double sum = (sh.red[0] + sh.red[1]) + (sh.red[2] + sh.red[3]);
        const int n_in = (sh.n_in[0] + sh.n_in[1]) + (sh.n_in[2] + sh.n_in[3]);
        usable[item] = n_u;
        status[item] = 0;
        sigma[item * 2 + 0] = s0;
        sigma[item * 2 + 1] = n_in > 5 ? sqrt(sum / (double)(n_in - 5)) : nan64();
    }
    if (tid < Q) quant[item * Q + tid] = __longlong_as_double((long long)sh.sel.prefix[tid]);
    if (tid < T) within[item * T + tid] = sh.within[tid];
}

bool in_range(int v) { return v >= 1 && v <= CPN_POSE_EVAL_MAX; }

}  // namespace

extern "C" int cpn_pose_errors(const float* poses, const float* gt, int B, int P, double* out, void* stream) {
    CPN_REQUIRE(poses && gt && out, CPN_E_ARG, "cpn_pose_errors: null pointer");
    CPN_REQUIRE(B >= 1 && B <= 32767 && in_range(P), CPN_E_SHAPE, "cpn_pose_errors: need 1 <= B <= 32767 pairs of 1 <= P <= %d poses (got B %d, P %d)",
                CPN_POSE_EVAL_MAX, B, P);
    hipLaunchKernelGGL(pose_errors_kernel, dim3(cpn_cdiv((long long)B * P, NT)), dim3(NT), 0, (hipStream_t)stream, poses, gt, B, P, out);
    CPN_LAUNCH_CHECK("cpn_pose_errors");
    return 0;
}

extern "C" int cpn_residual_stats(const float* xy, const int* count, const float* intrinsics, const float* poses, const double* q,
                                  const double* thr, int B, int N, int P, int Q, int T, int* usable, double* quant, int* within,
                                  double* sigma, int* status, void* stream) {
    CPN_REQUIRE(xy && count && intrinsics && poses && q && thr && usable && quant && within && sigma && status, CPN_E_ARG,
                "cpn_residual_stats: null pointer");
    CPN_REQUIRE(B >= 1 && B <= 32767 && N >= 1 && N <= (1 << 24) && in_range(P) && in_range(Q) && in_range(T), CPN_E_SHAPE,
                "cpn_residual_stats: need 1 <= B <= 32767, 1 <= N <= 2^24 and 1 <= P, Q, T <= %d (got B %d, N %d, P %d, Q %d, T %d)",
                CPN_POSE_EVAL_MAX, B, N, P, Q, T);
    StatArgs args = {};
    args.Q = Q;
    args.T = T;
    for (int j = 0; j < Q; ++j) {
        CPN_REQUIRE(q[j] >= 0.0 && q[j] <= 1.0, CPN_E_ARG, "cpn_residual_stats: q[%d] = %g is not in [0, 1]", j, q[j]);
        args.q[j] = q[j];
    }
    for (int t = 0; t < T; ++t) {
        CPN_REQUIRE(px_ok(thr[t]), CPN_E_ARG, "cpn_residual_stats: thr[%d] = %g is not finite and >= 0", t, thr[t]);
        args.thr[t] = thr[t];
    }
    hipLaunchKernelGGL(residual_stats_kernel, dim3(P, B), dim3(NT), 0, (hipStream_t)stream, xy, count, intrinsics, poses, args, N, usable,
                       quant, within, sigma, status);
    CPN_LAUNCH_CHECK("cpn_residual_stats");
    return 0;
}
