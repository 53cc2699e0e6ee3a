// Two photos in, their dense correspondences out (coponerf_amd/matches.py): the consumer of the two flows get_z returns.
//
//   match_fields_kernel       cpn_match_fields: one thread per (direction, pair, pixel) of the S x S grid (32 x 8 tiles; item =
//                             d B + b): the match q = p + up_flow(p), the cycle error cycle_masks thresholds (flow_warp.h's fp32
//                             sequence, the four taps of the other direction's flow formed as F.interpolate forms them), the
//                             in-image test and the signed Sampson residual of the pair under rel_pose in float64.
//   matches_count_kernel /    cpn_compact_matches: compact.h's two launches over a pair's (direction, row, column) sequence; a
//   matches_write_kernel      kept match writes (x0, y0, x1, y1) - view 0's point first - and (cycle, epi).
//   refine_pose_kernel        cpn_refine_pose: ONE workgroup of 256 threads per pair, all Gauss-Newton iterations inside it:
//                             pose_gauss_newton.h's passes (ransac.hip's polish shares them) from rel_pose.  No partials in HBM,
//                             no inter-workgroup synchronisation.
//
// The residual is float64 from the fp32 inputs, one rounding per operation (-ffp-contract=off), sums left to right:
// tests/matches_ref.py restates all three in numpy.  Cam and Pose are pinhole.h's; essential, sampson and residual_ok are sampson.h's,
// the use of rel_pose and the pose written out pose_out.h's, the count clamp ransac_common.h's: ransac.hip shares all three.
// cross_rows and the Rodrigues step are rotation_step.h's and the Cholesky solve cholesky_solve.h's: model_select.hip shares both.
#include "common.h"
#include "compact.h"
#include "flow_warp.h"
#include "pinhole.h"
#include "pose_gauss_newton.h"
#include "pose_out.h"
#include "ransac_common.h"
#include "sampson.h"

#include <math.h>

namespace {

constexpr int NT = 256;
constexpr int PTW = 32, PTH = NT / PTW;                    // match fields: the tile of one workgroup

__global__ __launch_bounds__(NT) void match_fields_kernel(const float* __restrict__ flow0, const float* __restrict__ flow1,
                                                          const float* __restrict__ intrinsics, const float* __restrict__ rel_pose,
                                                          int B, int S, int h, float fs, float rs, float* __restrict__ q,
                                                          float* __restrict__ cycle, float* __restrict__ epi,
                                                          uint8_t* __restrict__ inside) {
    const int tid = threadIdx.x;
    const int gx = blockIdx.x * PTW + (tid & (PTW - 1)), gy = blockIdx.y * PTH + tid / PTW;
    if (gx >= S || gy >= S) return;
    const int item = blockIdx.z, d = item / B, b = item - d * B;
    const float* const own = (d ? flow1 : flow0) + (size_t)b * 2 * h * h;
    const float* const oth = (d ? flow0 : flow1) + (size_t)b * 2 * h * h;

    float ux, uy, ix, iy;
    up_flow(own, h, h, fs, rs, gx, gy, ux, uy);
    warp_coord(S, S, gx, gy, ux, uy, ix, iy);
    const WarpTaps t = warp_taps(ix, iy, S, S);
    const float wt[4] = {t.wx0 * t.wy0, t.wx1 * t.wy0, t.wx0 * t.wy1, t.wx1 * t.wy1};
    const bool ok[4] = {t.vy0 && t.vx0, t.vy0 && t.vx1, t.vy1 && t.vx0, t.vy1 && t.vx1};
    const int tx[4] = {t.x0, t.x1, t.x0, t.x1}, ty[4] = {t.y0, t.y0, t.y1, t.y1};
    // warp(up_other, up_own): grid_sample's sum over the taps in its order (cpn_flow_panels' expression)
    float cx = 0.f, cy = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (ok[k]) {
            float ox, oy;
            up_flow(oth, h, h, fs, rs, tx[k], ty[k], ox, oy);
            cx += ox * wt[k];
            cy += oy * wt[k];
        }
    }
    const float ex = ux + cx, ey = uy + cy;
    const float norm = sqrtf(ex * ex + ey * ey);
    const float mx = ux + (float)gx, my = uy + (float)gy, hi = (float)(S - 1);
    const bool in = mx >= 0.f && mx <= hi && my >= 0.f && my <= hi;

    // the pair as (view 0's point, view 1's point)
    const double px = (double)gx, py = (double)gy, qx = (double)mx, qy = (double)my;
    const Cam k0 = load_cam(intrinsics + ((size_t)b * 2 + 0) * 16), k1 = load_cam(intrinsics + ((size_t)b * 2 + 1) * 16);
    const Pose rel = load_pose(rel_pose + (size_t)b * 16);
    double E[9];
    essential(&rel.R[0][0], rel.t, E);
    const Sampson s = d ? sampson(E, k0, k1, qx, qy, px, py) : sampson(E, k0, k1, px, py, qx, qy);
    const double res = s.n / sqrt(s.D);
    const float e32 = residual_ok(s, res) ? (float)res : __builtin_nanf("");

    const size_t at = ((size_t)item * S + gy) * S + gx;
    q[2 * at + 0] = mx;
    q[2 * at + 1] = my;
    cycle[at] = norm;
    epi[at] = e32;
    inside[at] = in ? 1 : 0;
}

// ---- compaction (compact.h): what a kept match writes
__global__ __launch_bounds__(NT) void matches_count_kernel(const uint8_t* __restrict__ keep, int B, int SS, int cap,
                                                           int* __restrict__ counts) {
    const int b = blockIdx.y;
    const int n = compact_tile_count(cap, [&](int j) { return keep[seq_source(j, b, B, SS)] != 0; });
    if (threadIdx.x == 0) counts[(size_t)b * gridDim.x + blockIdx.x] = n;
}

__global__ __launch_bounds__(NT) void matches_write_kernel(const uint8_t* __restrict__ keep, const float* __restrict__ q,
                                                           const float* __restrict__ cycle, const float* __restrict__ epi, int B,
                                                           int S, int cap, const int* __restrict__ counts, float* __restrict__ xy,
                                                           float* __restrict__ err, int* __restrict__ count) {
    const int b = blockIdx.y, SS = S * S;
    const int at = compact_tile_rows(
        counts + (size_t)b * gridDim.x, cap, [&](int j) { return keep[seq_source(j, b, B, SS)] != 0; },
        [&](int j, int row) {
            const int d = j / SS, p = j - d * SS, gy = p / S, gx = p - gy * S;
            const size_t in = (size_t)seq_source(j, b, B, SS), o = (size_t)b * cap + (size_t)row;
            const float px = (float)gx, py = (float)gy, qx = q[2 * in + 0], qy = q[2 * in + 1];
            xy[4 * o + 0] = d ? qx : px;
            xy[4 * o + 1] = d ? qy : py;
            xy[4 * o + 2] = d ? px : qx;
            xy[4 * o + 3] = d ? py : qy;
            err[2 * o + 0] = cycle[in];
            err[2 * o + 1] = epi[in];
        });
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) count[b] = at;
}

// ---- refinement: pose_gauss_newton.h's passes from rel_pose
__global__ __launch_bounds__(NT) void refine_pose_kernel(const float* __restrict__ xy, const int* __restrict__ count,
                                                         const float* __restrict__ intrinsics, const float* __restrict__ rel_pose,
                                                         int N, int iters, double scale_px, float* __restrict__ pose,
                                                         double* __restrict__ stats) {
    __shared__ RefineState st;
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* const P = rel_pose + (size_t)b * 16;
    const int n = clamp_count(count[b], N);
    double len0 = 0.0;
    if (tid == 0) {
        const RelStart start = rel_start(P);
        len0 = start.len0;
        st.go = (start.ok && n > 0 && iters > 0) ? 1 : 0;
        for (int r = 0; r < 3; ++r)                         // whether or not the pair goes on, as ever: the compiler's schedule
            for (int c = 0; c < 3; ++c) st.R[3 * r + c] = start.rel.R[r][c];        // of the match loop turns on it
        if (st.go) {
            for (int r = 0; r < 3; ++r) st.t[r] = start.rel.t[r] / len0;
            set_matrices(st);
        }
    }
    __syncthreads();
    if (!st.go) {                                          // nothing to do: rel_pose as it came, status 2
        if (tid < 16) pose[(size_t)b * 16 + tid] = P[tid];
        if (tid < 8) stats[(size_t)b * 8 + tid] = tid == 7 ? 2.0 : 0.0;
        return;
    }
    const Cam k0 = load_cam(intrinsics + ((size_t)b * 2 + 0) * 16), k1 = load_cam(intrinsics + ((size_t)b * 2 + 1) * 16);
    pose_passes(st, xy + (size_t)b * N * 4, n, k0, k1, iters, scale_px,
                [&](double cost0, const double (&sum)[POSE_NSUM], int done, int status) {
                    double deg_R, deg_t;
                    pose_angles(st.R, st.t, load_pose(P), len0, deg_R, deg_t);     // rel_pose read again: not held over the passes
                    store_pose(pose + (size_t)b * 16, st.R, st.t, len0);
                    double* const so = stats + (size_t)b * 8;
                    so[0] = cost0;
                    so[1] = sum[27];
                    so[2] = sum[28];
                    so[3] = sum[29];
                    so[4] = deg_R;
                    so[5] = deg_t;
                    so[6] = (double)done;
                    so[7] = (double)status;
                });
}

bool grid_ok(int B, int S) { return B >= 1 && B <= 32767 && S >= 1 && S <= 16384 && 2LL * B * S * S < (1LL << 31); }

}  // namespace

extern "C" int cpn_match_fields(const float* flow0, const float* flow1, const float* intrinsics, const float* rel_pose, int B, int S,
                                int h, float* q, float* cycle, float* epi, uint8_t* inside, void* stream) {
    CPN_REQUIRE(flow0 && flow1 && intrinsics && rel_pose && q && cycle && epi && inside, CPN_E_ARG, "cpn_match_fields: null pointer");
    CPN_REQUIRE(grid_ok(B, S) && h >= 1 && S % h == 0, CPN_E_SHAPE,
                "cpn_match_fields: need 1 <= B <= 32767, S a multiple of h >= 1, S <= 16384 and 2 B S S < 2^31 (got B %d, S %d, h %d)", B,
                S, h);
    const float fs = (float)((double)S / (double)h);       // the Python float S / h, rounded when it meets the fp32 tensor
    const float rs = (float)h / (float)S;                  // ATen's area_pixel_compute_scale in fp32
    const dim3 grid(cpn_cdiv(S, PTW), cpn_cdiv(S, PTH), 2 * B);
    hipLaunchKernelGGL(match_fields_kernel, grid, dim3(NT), 0, (hipStream_t)stream, flow0, flow1, intrinsics, rel_pose, B, S, h, fs, rs,
                       q, cycle, epi, inside);
    CPN_LAUNCH_CHECK("cpn_match_fields");
    return 0;
}

extern "C" int cpn_compact_matches_scratch(int B, int S) {
    if (!grid_ok(B, S)) return 0;
    return (int)((long long)B * cpn_cdiv(2LL * S * S, CPN_COMPACT_TILE));
}

extern "C" int cpn_compact_matches(const uint8_t* keep, const float* q, const float* cycle, const float* epi, int B, int S,
                                   int* scratch, float* xy, float* err, int* count, void* stream) {
    CPN_REQUIRE(keep && q && cycle && epi && scratch && xy && err && count, CPN_E_ARG, "cpn_compact_matches: null pointer");
    CPN_REQUIRE(grid_ok(B, S), CPN_E_SHAPE, "cpn_compact_matches: need 1 <= B <= 32767, 1 <= S <= 16384 and 2 B S S < 2^31 (got B %d, S %d)",
                B, S);
    const int SS = S * S, cap = 2 * SS;
    const dim3 grid(cpn_cdiv(cap, CPN_COMPACT_TILE), B);
    hipLaunchKernelGGL(matches_count_kernel, grid, dim3(NT), 0, (hipStream_t)stream, keep, B, SS, cap, scratch);
    CPN_LAUNCH_CHECK("cpn_compact_matches (count)");
    hipLaunchKernelGGL(matches_write_kernel, grid, dim3(NT), 0, (hipStream_t)stream, keep, q, cycle, epi, B, S, cap, (const int*)scratch,
                       xy, err, count);
    CPN_LAUNCH_CHECK("cpn_compact_matches (write)");
    return 0;
}

extern "C" int cpn_refine_pose(const float* xy, const int* count, const float* intrinsics, const float* rel_pose, int B, int N,
                               int iters, double scale_px, float* pose, double* stats, void* stream) {
    CPN_REQUIRE(xy && count && intrinsics && rel_pose && pose && stats, CPN_E_ARG, "cpn_refine_pose: null pointer");
    CPN_REQUIRE(B >= 1 && N >= 1, CPN_E_SHAPE, "cpn_refine_pose: need B >= 1 pairs of N >= 1 rows (got B %d, N %d)", B, N);
    CPN_REQUIRE(iters >= 0 && scale_px > 0.0 && scale_px <= 1.79769313486231570815e308, CPN_E_ARG,
                "cpn_refine_pose: need iters >= 0 and a finite scale_px > 0 (got %d, %g)", iters, scale_px);
    hipLaunchKernelGGL(refine_pose_kernel, dim3(B), dim3(NT), 0, (hipStream_t)stream, xy, count, intrinsics, rel_pose, N, iters,
                       scale_px, pose, stats);
    CPN_LAUNCH_CHECK("cpn_refine_pose");
    return 0;
}
