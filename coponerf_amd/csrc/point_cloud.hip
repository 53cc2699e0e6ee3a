// Two photos in, a fused coloured point cloud out (coponerf_amd/point_cloud.py): the per-pixel geometry behind render_path's depth.
//
//   depth_points_kernel       cpn_depth_points: one thread per (view, pair, pixel): pose . (d . ray) in the reference frame.
//   depth_votes_kernel        cpn_depth_votes: one thread per (view a, pair, pixel): for every other view b in ascending order the
//                             point goes into b, b's depth is read bilinearly there, the point of that depth comes back into a;
//                             a vote where it lands within px_tol pixels and rel_tol . d_a of where it started.
//   compact_count_kernel /    cpn_compact_points: a workgroup owns CPN_COMPACT_TILE consecutive elements of a pair's (view, row,
//   compact_write_kernel      column) sequence.  The first launch counts the selected ones per workgroup; the second adds the counts
//                             of the workgroups before its own, ranks its own elements by wave ballots and writes: compact.h,
//                             shared with matches.hip.  No atomics: an element's output row depends on the mask alone.
//
// The geometry (pinhole.h's camera) is float64 from the fp32 inputs, one rounding per operation (-ffp-contract=off), sums left
// to right, and one rounding to fp32 at the store: tests/point_cloud_ref.py restates it in numpy.
#include "common.h"
#include "byte_pack.h"
#include "compact.h"
#include "pinhole.h"

#include <math.h>

namespace {

constexpr int NT = 256;
constexpr int TILE = CPN_COMPACT_TILE;
static_assert(COMPACT_NT == NT, "the compaction kernels run 256 threads");

// element i = (view k, pair b, pixel p) of the (K, B, h w) arrays
struct Elem {
    int kb, k, b, r, c;
};
__device__ __forceinline__ Elem elem_of(int i, int B, int hw, int w) {
    Elem e;
    e.kb = i / hw;
    const int p = i - e.kb * hw;
    e.k = e.kb / B;
    e.b = e.kb - e.k * B;
    e.r = p / w;
    e.c = p - e.r * w;
    return e;
}

__global__ __launch_bounds__(NT) void depth_points_kernel(const float* __restrict__ depth, const float* __restrict__ poses,
                                                          const float* __restrict__ intrinsics, int total, int B, int y0, int x0,
                                                          int hw, int w, float* __restrict__ xyz) {
    const int i = blockIdx.x * NT + threadIdx.x;           // total < 2^31: the entry point checks it
    if (i >= total) return;
    float* const o = xyz + (size_t)i * 3;
    const float d = depth[i];
    if (!depth_valid(d)) {
        o[0] = o[1] = o[2] = __builtin_nanf("");
        return;
    }
    const Elem e = elem_of(i, B, hw, w);
    const Cam cam = load_cam(intrinsics + (size_t)e.b * 16);
    const Pose P = load_pose(poses + (size_t)e.kb * 16);
    double p[3], X[3];
    on_ray(cam, (double)(x0 + e.c), (double)(y0 + e.r), (double)d, p);
    to_reference(P, p, X);
    o[0] = (float)X[0];
    o[1] = (float)X[1];
    o[2] = (float)X[2];
}

__global__ __launch_bounds__(NT) void depth_votes_kernel(const float* __restrict__ depth, const float* __restrict__ poses,
                                                         const float* __restrict__ intrinsics, int total, int K, int B, int y0,
                                                         int x0, int h, int w, double px_tol, double rel_tol,
                                                         uint8_t* __restrict__ votes, float* __restrict__ fused) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= total) return;
    const float da32 = depth[i];
    if (!depth_valid(da32)) {
        votes[i] = 0;
        fused[i] = __builtin_nanf("");
        return;
    }
    const int hw = h * w;
    const Elem e = elem_of(i, B, hw, w);
    const Cam cam = load_cam(intrinsics + (size_t)e.b * 16);
    const Pose Pa = load_pose(poses + (size_t)e.kb * 16);
    const double da = (double)da32, u = (double)(x0 + e.c), v = (double)(y0 + e.r);
    double p[3], X[3];
    on_ray(cam, u, v, da, p);
    to_reference(Pa, p, X);
    double sum = da;
    int n = 0;
    for (int kb = 0; kb < K; ++kb) {
        if (kb == e.k) continue;
        const Pose Pb = load_pose(poses + ((size_t)kb * B + e.b) * 16);
        double Y[3], qx, qy;
        to_camera(Pb, X, Y);
        if (!(Y[2] > 0.0)) continue;                       // behind view b
        project(cam, Y, qx, qy);
        const double wx = qx - (double)x0, wy = qy - (double)y0;               // window coordinates
        if (!(wx >= 0.0 && wx < (double)(w - 1) && wy >= 0.0 && wy < (double)(h - 1))) continue;      // a tap outside (or NaN)
        const int ix = (int)wx, iy = (int)wy;              // 0 <= ix <= w - 2, 0 <= iy <= h - 2: the four taps lie inside
        const float* const D = depth + ((size_t)kb * B + e.b) * hw + (size_t)iy * w + ix;
        const float d00 = D[0], d01 = D[1], d10 = D[w], d11 = D[w + 1];
        if (!(depth_valid(d00) && depth_valid(d01) && depth_valid(d10) && depth_valid(d11))) continue;
        const double ax = wx - (double)ix, ay = wy - (double)iy;
        const double db = (1.0 - ay) * ((1.0 - ax) * (double)d00 + ax * (double)d01) +
                          ay * ((1.0 - ax) * (double)d10 + ax * (double)d11);
        double X2[3], Y2[3], bx, by;
        on_ray(cam, qx, qy, db, p);
        to_reference(Pb, p, X2);
        to_camera(Pa, X2, Y2);
        if (!(Y2[2] > 0.0)) continue;                      // came back behind view a: no pixel to compare
        project(cam, Y2, bx, by);
        const double ex = bx - u, ey = by - v;
        if (sqrt(ex * ex + ey * ey) <= px_tol && fabs(Y2[2] - da) <= rel_tol * da) {
            sum += Y2[2];
            ++n;
        }
    }
    votes[i] = (uint8_t)n;                                 // n <= K - 1 <= 254
    fused[i] = (float)(sum / (double)(1 + n));
}

// ---- compaction (compact.h): what a selected point writes
__global__ __launch_bounds__(NT) void compact_count_kernel(const uint8_t* __restrict__ keep, int B, int hw, int cap,
                                                           int* __restrict__ counts) {
    const int b = blockIdx.y;
    const int n = compact_tile_count(cap, [&](int j) { return keep[seq_source(j, b, B, hw)] != 0; });
    if (threadIdx.x == 0) counts[(size_t)b * gridDim.x + blockIdx.x] = n;
}

__global__ __launch_bounds__(NT) void compact_write_kernel(const uint8_t* __restrict__ keep, const float* __restrict__ xyz,
                                                           const float* __restrict__ rgb, int B, int hw, int cap,
                                                           const int* __restrict__ counts, float* __restrict__ out_xyz,
                                                           uint8_t* __restrict__ out_rgb, int* __restrict__ count) {
    const int b = blockIdx.y;
    const int at = compact_tile_rows(
        counts + (size_t)b * gridDim.x, cap, [&](int j) { return keep[seq_source(j, b, B, hw)] != 0; },
        [&](int j, int row) {
            const size_t o = ((size_t)b * cap + (size_t)row) * 3, in = (size_t)seq_source(j, b, B, hw) * 3;
            for (int c = 0; c < 3; ++c) {
                out_xyz[o + c] = xyz[in + c];
                out_rgb[o + c] = to_byte((rgb[in + c] + 1.0f) * 127.5f);
            }
        });
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) count[b] = at;
}

bool grid_ok(int K, int B, int h, int w) {
    return K >= 1 && K <= 255 && B >= 1 && h >= 1 && w >= 1 && (long long)K * B * h * w < (1LL << 31);
}

int check_views(const char* who, int K, int B, int S, int y0, int x0, int h, int w) {
    CPN_REQUIRE(grid_ok(K, B, h, w), CPN_E_SHAPE,
                "%s: need 1 <= K <= 255 views, B, h, w >= 1 and K B h w < 2^31 (got K %d, B %d, h %d, w %d)", who, K, B, h, w);
    CPN_REQUIRE(S >= 1 && y0 >= 0 && x0 >= 0 && y0 <= S - h && x0 <= S - w, CPN_E_SHAPE,
                "%s: the window (%d, %d, %d, %d) does not lie in the %d x %d grid", who, y0, x0, h, w, S, S);
    return 0;
}

}  // namespace

extern "C" int cpn_depth_points(const float* depth, const float* poses, const float* intrinsics, int K, int B, int S, int y0, int x0,
                                int h, int w, float* xyz, void* stream) {
    CPN_REQUIRE(depth && poses && intrinsics && xyz, CPN_E_ARG, "cpn_depth_points: null pointer");
    if (const int bad = check_views("cpn_depth_points", K, B, S, y0, x0, h, w)) return bad;
    const int total = K * B * h * w;
    hipLaunchKernelGGL(depth_points_kernel, dim3(cpn_cdiv(total, NT)), dim3(NT), 0, (hipStream_t)stream, depth, poses, intrinsics,
                       total, B, y0, x0, h * w, w, xyz);
    CPN_LAUNCH_CHECK("cpn_depth_points");
    return 0;
}

extern "C" int cpn_depth_votes(const float* depth, const float* poses, const float* intrinsics, int K, int B, int S, int y0, int x0,
                               int h, int w, double px_tol, double rel_tol, uint8_t* votes, float* depth_fused, void* stream) {
    CPN_REQUIRE(depth && poses && intrinsics && votes && depth_fused, CPN_E_ARG, "cpn_depth_votes: null pointer");
    if (const int bad = check_views("cpn_depth_votes", K, B, S, y0, x0, h, w)) return bad;
    CPN_REQUIRE(px_tol >= 0.0 && rel_tol >= 0.0, CPN_E_ARG, "cpn_depth_votes: px_tol and rel_tol must be >= 0 (got %g, %g)", px_tol,
                rel_tol);
    const int total = K * B * h * w;
    hipLaunchKernelGGL(depth_votes_kernel, dim3(cpn_cdiv(total, NT)), dim3(NT), 0, (hipStream_t)stream, depth, poses, intrinsics,
                       total, K, B, y0, x0, h, w, px_tol, rel_tol, votes, depth_fused);
    CPN_LAUNCH_CHECK("cpn_depth_votes");
    return 0;
}

extern "C" int cpn_compact_points_scratch(int K, int B, int h, int w) {
    if (!grid_ok(K, B, h, w) || B > 65535) return 0;
    return (int)((long long)B * cpn_cdiv((long long)K * h * w, TILE));
}

extern "C" int cpn_compact_points(const uint8_t* keep, const float* xyz, const float* rgb, int K, int B, int h, int w, int* scratch,
                                  float* out_xyz, uint8_t* out_rgb, int* count, void* stream) {
    CPN_REQUIRE(keep && xyz && rgb && scratch && out_xyz && out_rgb && count, CPN_E_ARG, "cpn_compact_points: null pointer");
    CPN_REQUIRE(grid_ok(K, B, h, w) && B <= 65535, CPN_E_SHAPE,
                "cpn_compact_points: need 1 <= K <= 255 views, 1 <= B <= 65535, h, w >= 1 and K B h w < 2^31 (got K %d, B %d, h %d, w %d)",
                K, B, h, w);
    const int hw = h * w, cap = K * hw;
    const dim3 grid(cpn_cdiv(cap, TILE), B);
    hipLaunchKernelGGL(compact_count_kernel, grid, dim3(NT), 0, (hipStream_t)stream, keep, B, hw, cap, scratch);
    CPN_LAUNCH_CHECK("cpn_compact_points (count)");
    hipLaunchKernelGGL(compact_write_kernel, grid, dim3(NT), 0, (hipStream_t)stream, keep, xyz, rgb, B, hw, cap, (const int*)scratch,
                       out_xyz, out_rgb, count);
    CPN_LAUNCH_CHECK("cpn_compact_points (write)");
    return 0;
}
