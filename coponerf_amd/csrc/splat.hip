// A PointCloud drawn into any camera through a z-buffer (coponerf_amd/splat.py): the one result of the package a user could
// not look at on a headless machine, and a check of depth and pose against the second photo that needs no ground truth.
//
//   splat_points_kernel       cpn_splat_points: one thread per (camera, pair, point): the point goes into the camera, its
//                             footprint takes the minimum of (depth bits, index) per pixel by a 64-bit integer atomic minimum.
//   splat_resolve_kernel      cpn_splat_resolve: one thread per output pixel: its key (or, with fill, the smallest key of its
//                             neighbourhood) becomes index, depth and colour.
//   splat_score_kernel /      cpn_splat_score: a workgroup counts the covered pixels of SCORE_TILE pixels of an image and adds
//   splat_score_finish_kernel their squared byte differences; the second launch adds an image's workgroups.  Integers: exact.
//
// The atomic minimum is the library's first atomic on a result path.  It keeps the rule that two runs give the same bytes: the
// minimum of a set of integers does not depend on the order in which they arrive (include/coponerf_hip.h).
// The key, its minimum and a resolved pixel's stores are zbuffer.h's, shared with raster.hip.  The camera is pinhole.h's: float64
// from the fp32 inputs, one rounding per operation (-ffp-contract=off), sums left to right: tests/splat_ref.py restates it.
#include "common.h"
#include "pinhole.h"
#include "zbuffer.h"

#include <math.h>

namespace {

constexpr int NT = 256;
constexpr int SCORE_TILE = CPN_SPLAT_SCORE_TILE;           // pixels of one image per workgroup of the score
static_assert(SCORE_TILE % NT == 0, "a thread of the score walks SCORE_TILE / 256 pixels");

__global__ __launch_bounds__(NT) void splat_points_kernel(const float* __restrict__ xyz, const int* __restrict__ count,
                                                          const float* __restrict__ poses, const float* __restrict__ intrinsics,
                                                          int B, int cap, int tiles, int H, int W, int radius, double near,
                                                          unsigned long long* zbuf) {
    const int kb = blockIdx.x / tiles;                     // (camera k, pair b) = kb, uniform in the workgroup
    const int i = (blockIdx.x - kb * tiles) * NT + threadIdx.x;
    const int b = kb % B;
    if (i >= min(max(count[b], 0), cap)) return;           // rows beyond the count are never read
    const Pose P = load_pose(poses + (size_t)kb * 16);
    const Cam cam = load_cam(intrinsics + (size_t)b * 16);
    const float* const x = xyz + ((size_t)b * cap + (size_t)i) * 3;
    const double X[3] = {(double)x[0], (double)x[1], (double)x[2]};
    if (!(pose_finite(P) && finite3(X[0], X[1], X[2]) && cam_finite(cam))) return;
    double Y[3], u, v;
    to_camera_centred(P, X, Y);
    if (!(Y[2] >= near)) return;                           // behind the camera, nearer than near, or NaN
    project(cam, Y, u, v);
    const float z32 = (float)Y[2];
    constexpr double LIM = 1073741824.0;                   // 2^30: the pixel and its footprint fit an int
    if (!(fabs(u) < LIM && fabs(v) < LIM && isfinite(z32))) return;
    const int c = (int)floor(u + 0.5), r = (int)floor(v + 0.5);
    const int c0 = max(c - radius, 0), c1 = min(c + radius, W - 1), r0 = max(r - radius, 0), r1 = min(r + radius, H - 1);
    const unsigned long long key = zbuf_key(z32, (unsigned)i);
    unsigned long long* const Z = zbuf + (size_t)kb * H * W;
    for (int rr = r0; rr <= r1; ++rr) {                    // an empty range where the footprint misses the image
        for (int cc = c0; cc <= c1; ++cc) zbuf_min(Z + (size_t)rr * W + cc, key);
    }
}

__global__ __launch_bounds__(NT) void splat_resolve_kernel(const unsigned long long* __restrict__ zbuf,
                                                           const uint8_t* __restrict__ rgb, int total, int B, int cap, int H, int W,
                                                           int fill, int background, uint8_t* __restrict__ frames,
                                                           float* __restrict__ depth, int* __restrict__ index) {
    const int i = blockIdx.x * NT + threadIdx.x;           // total = K B H W < 2^31: the entry point checks it
    if (i >= total) return;
    const int hw = H * W, kb = i / hw, p = i - kb * hw, r = p / W, c = p - r * W;
    unsigned long long key = zbuf[i];
    if (key == ZBUF_EMPTY && fill > 0) {                   // the smallest key around it, of the buffer as it was splatted
        const unsigned long long* const Z = zbuf + (size_t)kb * hw;
        for (int rr = max(r - fill, 0); rr <= min(r + fill, H - 1); ++rr)
            for (int cc = max(c - fill, 0); cc <= min(c + fill, W - 1); ++cc) key = min(key, Z[(size_t)rr * W + cc]);
    }
    const bool hit = zbuf_hit(key, cap);
    uint8_t out[3];
    zbuf_background(background, out);
    if (hit) {
        const uint8_t* const col = rgb + ((size_t)(kb % B) * cap + zbuf_row(key)) * 3;
        for (int ch = 0; ch < 3; ++ch) out[ch] = col[ch];
    }
    zbuf_store(i, hit, key, out, frames, depth, index);
}

// partial (K B, tiles, 2): the covered pixels of the workgroup's SCORE_TILE pixels and their squared differences
__global__ __launch_bounds__(NT) void splat_score_kernel(const uint8_t* __restrict__ frames, const int* __restrict__ index,
                                                         const uint8_t* __restrict__ target, int hw, int tiles,
                                                         long long* __restrict__ partial) {
    const int kb = blockIdx.x / tiles, p0 = (blockIdx.x - kb * tiles) * SCORE_TILE;
    long long s[2] = {0, 0};
    for (int j = threadIdx.x; j < min(SCORE_TILE, hw - p0); j += NT) {
        const size_t at = (size_t)kb * hw + p0 + j;        // K B H W < 2^31
        if (index[at] < 0) continue;
        s[0] += 1;
        for (int ch = 0; ch < 3; ++ch) {
            const int e = (int)frames[at * 3 + ch] - (int)target[at * 3 + ch];
            s[1] += e * e;
        }
    }
    block256_sum(s);
    if (threadIdx.x == 0) {
        partial[(size_t)blockIdx.x * 2] = s[0];
        partial[(size_t)blockIdx.x * 2 + 1] = s[1];
    }
}

// sum_counts_256's walk on the int64 pairs: thread t adds the workgroups t, t + 256, .. of its image, block256_sum the threads
__global__ __launch_bounds__(NT) void splat_score_finish_kernel(const long long* __restrict__ partial, int tiles,
                                                                long long* __restrict__ stats) {
    const long long* const p = partial + (size_t)blockIdx.x * tiles * 2;
    long long s[2] = {0, 0};
    for (int i = threadIdx.x; i < tiles; i += NT) {
        s[0] += p[2 * i];
        s[1] += p[2 * i + 1];
    }
    block256_sum(s);
    if (threadIdx.x == 0) {
        stats[(size_t)blockIdx.x * 2] = s[0];
        stats[(size_t)blockIdx.x * 2 + 1] = s[1];
    }
}

long long score_tiles(int H, int W) { return cpn_cdiv((long long)H * W, SCORE_TILE); }

}  // namespace

extern "C" int cpn_splat_points(const float* xyz, const int* count, const float* poses, const float* intrinsics, int K, int B,
                                int cap, int H, int W, int radius, double near, unsigned long long* zbuf, void* stream) {
    CPN_REQUIRE(xyz && count && poses && intrinsics && zbuf, CPN_E_ARG, "cpn_splat_points: null pointer");
    if (const int bad = check_image("cpn_splat_points", K, B, H, W)) return bad;
    const long long tiles = cpn_cdiv(cap, NT);
    CPN_REQUIRE(cap >= 1 && (long long)K * B * tiles < (1LL << 31), CPN_E_SHAPE,
                "cpn_splat_points: need 1 <= cap < 2^31 and K B ceil(cap / 256) < 2^31 (got K %d, B %d, cap %d)", K, B, cap);
    CPN_REQUIRE(radius >= 0 && radius <= 8 && near > 0.0, CPN_E_ARG,
                "cpn_splat_points: need 0 <= radius <= 8 and near > 0 (got %d, %g)", radius, near);
    if (const int bad = zbuf_clear(zbuf, K, B, H, W, (hipStream_t)stream, "cpn_splat_points")) return bad;
    hipLaunchKernelGGL(splat_points_kernel, dim3((unsigned)(K * B * tiles)), dim3(NT), 0, (hipStream_t)stream, xyz, count, poses,
                       intrinsics, B, cap, (int)tiles, H, W, radius, near, zbuf);
    CPN_LAUNCH_CHECK("cpn_splat_points");
    return 0;
}

extern "C" int cpn_splat_resolve(const unsigned long long* zbuf, const uint8_t* rgb, int K, int B, int cap, int H, int W, int fill,
                                 int background, uint8_t* frames, float* depth, int* index, void* stream) {
    CPN_REQUIRE(zbuf && rgb && frames, CPN_E_ARG, "cpn_splat_resolve: null pointer");
    if (const int bad = check_image("cpn_splat_resolve", K, B, H, W)) return bad;
    CPN_REQUIRE(cap >= 1, CPN_E_SHAPE, "cpn_splat_resolve: need 1 <= cap < 2^31 (got %d)", cap);
    CPN_REQUIRE(fill >= 0 && fill <= 4 && background >= 0 && background <= 0xFFFFFF, CPN_E_ARG,
                "cpn_splat_resolve: need 0 <= fill <= 4 and background = r | g << 8 | b << 16 (got %d, %d)", fill, background);
    const int total = K * B * H * W;
    hipLaunchKernelGGL(splat_resolve_kernel, dim3(cpn_cdiv(total, NT)), dim3(NT), 0, (hipStream_t)stream, zbuf, rgb, total, B, cap,
                       H, W, fill, background, frames, depth, index);
    CPN_LAUNCH_CHECK("cpn_splat_resolve");
    return 0;
}

extern "C" int cpn_splat_score_scratch(int K, int B, int H, int W) {
    if (!image_ok(K, B, H, W)) return 0;
    return (int)(2 * (long long)K * B * score_tiles(H, W));      // <= 2 K B (H W / 2048 + 1) < 2^31
}

extern "C" int cpn_splat_score(const uint8_t* frames, const int* index, const uint8_t* target, int K, int B, int H, int W,
                               long long* scratch, long long* stats, void* stream) {
    CPN_REQUIRE(frames && index && target && scratch && stats, CPN_E_ARG, "cpn_splat_score: null pointer");
    if (const int bad = check_image("cpn_splat_score", K, B, H, W)) return bad;
    const int tiles = (int)score_tiles(H, W);
    hipLaunchKernelGGL(splat_score_kernel, dim3(K * B * tiles), dim3(NT), 0, (hipStream_t)stream, frames, index, target, H * W, tiles,
                       scratch);
    CPN_LAUNCH_CHECK("cpn_splat_score");
    hipLaunchKernelGGL(splat_score_finish_kernel, dim3(K * B), dim3(NT), 0, (hipStream_t)stream, (const long long*)scratch, tiles,
                       stats);
    CPN_LAUNCH_CHECK("cpn_splat_score (finish)");
    return 0;
}
