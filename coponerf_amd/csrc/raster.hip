// A Mesh's triangles drawn into any camera through a z-buffer (coponerf_amd/raster.py): the consumer coponerf_amd.mesh lacked.
// A surface drawn as its vertices has holes between the dots and shows what lies behind it; drawn as triangles it is closed
// where it is closed, and hides what it hides.
//
//   raster_faces_kernel    cpn_raster_faces: one thread per (camera, pair, face) sets the face up (face_setup) and walks its
//                          bounding box itself if that holds at most CPN_RASTER_SMALL pixels; the wave then takes its larger
//                          faces one at a time (ballot, lane reads of the setup) and its 64 lanes stride over the box.  At
//                          most CPN_RASTER_TILES workgroups per (camera, pair) stride over the faces up to nface: the launch
//                          is sized by the capacity, but a mesh with room to spare costs workgroups that leave at once.
//   raster_resolve_kernel  cpn_raster_resolve: one thread per output pixel repeats the setup of the face its key names and
//                          forms colour (the vertices' bytes, or a headlight), depth, index and weights.
//
// Coverage is integer arithmetic on vertices snapped to 1/256 pixel, so it is exact, does not depend on the order of a face's
// indices, and gives a pixel centre on an edge two faces share to exactly one of them (the top-left rule of
// include/coponerf_hip.h).  The depth is float64, one rounding per operation (-ffp-contract=off), on the vertices in a
// canonical order (the camera: pinhole.h); the key, its atomic minimum and a resolved pixel's stores are zbuffer.h's, shared
// with splat.hip.  tests/raster_ref.py restates all of it in numpy.
#include "common.h"
#include "pinhole.h"
#include "zbuffer.h"

#include <math.h>

namespace {

constexpr int NT = 256;
constexpr int SMALL = CPN_RASTER_SMALL;
constexpr int TILES = CPN_RASTER_TILES;                    // workgroups per (camera, pair) at the most
constexpr int MAX_SIDE = 16384;
static_assert(SMALL >= 1, "a face of one pixel takes the one-lane path");

struct Vertex {
    long long X, Y;                                        // snapped to 1/256 pixel
    double cam[3];                                         // in the camera's frame
    int row, slot;                                         // the row of xyz, and the position in the face's three indices
};

// a face ready to be drawn: the vertices in the CANONICAL order (ascending row of xyz, then the second and third swapped if the
// doubled area is negative), so that nothing below depends on the order of the face's three indices
struct Face {
    Vertex v[3];
    long long area;                                        // the doubled area in 1/256-pixel units squared, > 0
    bool front;                                            // the doubled area of the indices AS STORED is negative
};

// edge a -> b of a face of positive area, in the form w(c, r) = w00 + c sc + r sr at pixel (c, r): the value is >= 0 inside
struct Edge {
    long long w00, sc, sr;
    int bias;                                              // 0: the edge owns the pixel centres on it (top-left rule), 1: not
};

__device__ __forceinline__ void cswap(Vertex& a, Vertex& b, bool swap) {
    if (swap) {
        const Vertex t = a;
        a = b;
        b = t;
    }
}

__device__ __forceinline__ long long doubled_area(const Vertex& a, const Vertex& b, const Vertex& c) {
    return (b.X - a.X) * (c.Y - a.Y) - (b.Y - a.Y) * (c.X - a.X);        // every factor below 2^30 in magnitude
}

// The header's "drawable" face, with near > 0 (cpn_raster_faces) or near = 0 (cpn_raster_resolve: Y_z > 0).  `tri` points at the
// face's three indices, `xyz` at the pair's first vertex; nv = min(max(nvert[b], 0), capv).
__device__ __forceinline__ bool face_setup(const int* __restrict__ tri, const float* __restrict__ xyz, int nv,
                                           const float* __restrict__ P, const float* __restrict__ Kb, double near, Face& F) {
    const Pose pose = load_pose(P);
    const Cam cam = load_cam(Kb);
    if (!(pose_finite(pose) && cam_finite(cam))) return false;
    constexpr double LIM = 536870912.0;                    // 2^29: differences stay below 2^30 and their products below 2^60
    for (int j = 0; j < 3; ++j) {
        const int row = tri[j];
        if (row < 0 || row >= nv) return false;            // nothing is read through an index outside the pair's vertices
        const float* const x = xyz + (size_t)row * 3;
        double pt[3];
        for (int a = 0; a < 3; ++a) {
            pt[a] = (double)x[a];
            if (!isfinite(pt[a])) return false;
        }
        Vertex& v = F.v[j];
        to_camera_centred(pose, pt, v.cam);
        const double z = v.cam[2];
        if (!(z >= near && z > 0.0 && isfinite((float)z))) return false;        // no clipping: the face is dropped whole
        double u, w;
        project(cam, v.cam, u, w);
        const double X = floor(256.0 * u + 0.5), Y = floor(256.0 * w + 0.5);
        if (!(fabs(X) < LIM && fabs(Y) < LIM)) return false;                    // a NaN fails
        v.X = (long long)X;
        v.Y = (long long)Y;
        v.row = row;
        v.slot = j;
    }
    const long long stored = doubled_area(F.v[0], F.v[1], F.v[2]);
    if (stored == 0) return false;
    F.front = stored < 0;
    cswap(F.v[0], F.v[1], F.v[0].row > F.v[1].row);        // equal rows are equal points: the area was 0
    cswap(F.v[1], F.v[2], F.v[1].row > F.v[2].row);
    cswap(F.v[0], F.v[1], F.v[0].row > F.v[1].row);
    const long long area = doubled_area(F.v[0], F.v[1], F.v[2]);
    cswap(F.v[1], F.v[2], area < 0);
    F.area = area < 0 ? -area : area;
    return true;
}

// w_i belongs to vertex i: it is the edge function of the opposite edge, (1 -> 2), (2 -> 0), (0 -> 1)
__device__ __forceinline__ Edge edge_of(const Vertex& a, const Vertex& b) {
    const long long dx = b.X - a.X, dy = b.Y - a.Y;
    Edge e;
    e.w00 = dy * a.X - dx * a.Y;                           // dx (256 r - Y_a) - dy (256 c - X_a) at (0, 0)
    e.sc = -256 * dy;
    e.sr = 256 * dx;
    e.bias = (dy < 0 || (dy == 0 && dx > 0)) ? 0 : 1;
    return e;
}

__device__ __forceinline__ long long edge_at(const Edge& e, int c, int r) { return e.w00 + (long long)c * e.sc + (long long)r * e.sr; }

// q_i = w_i / z_i and their sum, left to right: what the depth, the weights and the colour share
__device__ __forceinline__ double weights(const long long (&w)[3], const double (&z)[3], double (&q)[3]) {
    for (int i = 0; i < 3; ++i) q[i] = (double)w[i] / z[i];
    return (q[0] + q[1]) + q[2];
}

// one pixel centre against one face: the top-left rule, the depth, the key, the minimum
__device__ __forceinline__ void cover(const Edge (&e)[3], const double (&z)[3], long long area, unsigned face, int c, int r,
                                      unsigned long long* __restrict__ Z, int W) {
    long long w[3];
    for (int i = 0; i < 3; ++i) w[i] = edge_at(e[i], c, r);
    if (((w[0] - e[0].bias) | (w[1] - e[1].bias) | (w[2] - e[2].bias)) < 0) return;
    double q[3];
    const double s = weights(w, z, q);
    const float z32 = (float)((double)area / s);
    zbuf_min(Z + (size_t)r * W + c, zbuf_key(z32, face));
}

__device__ __forceinline__ int clamped_count(const int* __restrict__ n, int b, int cap) { return min(max(n[b], 0), cap); }

__global__ __launch_bounds__(NT) void raster_faces_kernel(const float* __restrict__ xyz, const int* __restrict__ nvert,
                                                          const int* __restrict__ faces, const int* __restrict__ nface,
                                                          const float* __restrict__ poses, const float* __restrict__ intrinsics,
                                                          int B, int capv, int capf, int tiles, int H, int W, int cull, double near,
                                                          unsigned long long* zbuf) {
    const int kb = blockIdx.x / tiles;                     // (camera k, pair b) = kb, uniform in the workgroup
    const int b = kb % B;
    const int nf = clamped_count(nface, b, capf);          // rows beyond the count are never read
    unsigned long long* const Z = zbuf + (size_t)kb * H * W;
    const int lane = threadIdx.x & 63;
    // the pair's `tiles` workgroups stride over its faces: the trip count is the same for every thread of a workgroup
    for (long long base = (long long)(blockIdx.x - kb * tiles) * NT; base < nf; base += (long long)tiles * NT) {
        const int f = (int)(base + threadIdx.x);           // beyond nf it is not used
        // no thread leaves before the wave's ballot: a face that is not drawn has a box of 0 pixels
        Face F;
        bool ok = base + threadIdx.x < nf;
        if (ok)
            ok = face_setup(faces + ((size_t)b * capf + (size_t)f) * 3, xyz + (size_t)b * capv * 3, clamped_count(nvert, b, capv),
                            poses + (size_t)kb * 16, intrinsics + (size_t)b * 16, near, F);
        ok = ok && (cull == 0 || F.front);
        Edge e[3] = {};
        double z[3] = {};
        long long area = 0;
        int c0 = 0, r0 = 0, bw = 0, n = 0;
        if (ok) {
            const long long loX = min(F.v[0].X, min(F.v[1].X, F.v[2].X)), hiX = max(F.v[0].X, max(F.v[1].X, F.v[2].X));
            const long long loY = min(F.v[0].Y, min(F.v[1].Y, F.v[2].Y)), hiY = max(F.v[0].Y, max(F.v[1].Y, F.v[2].Y));
            // the pixel centres 256 c in [lo, hi]: ceil and floor of a division by 256, as arithmetic shifts
            c0 = (int)max((loX + 255) >> 8, 0LL);
            r0 = (int)max((loY + 255) >> 8, 0LL);
            const int c1 = (int)min(hiX >> 8, (long long)(W - 1)), r1 = (int)min(hiY >> 8, (long long)(H - 1));
            if (c1 >= c0 && r1 >= r0) {
                bw = c1 - c0 + 1;
                n = bw * (r1 - r0 + 1);                    // <= H W <= 2^28
            }
            e[0] = edge_of(F.v[1], F.v[2]);
            e[1] = edge_of(F.v[2], F.v[0]);
            e[2] = edge_of(F.v[0], F.v[1]);
            for (int i = 0; i < 3; ++i) z[i] = F.v[i].cam[2];
            area = F.area;
        }
        if (n > 0 && n <= SMALL) {
            int c = c0, r = r0;
            for (int p = 0; p < n; ++p) {
                cover(e, z, area, (unsigned)f, c, r, Z, W);
                if (++c == c0 + bw) {
                    c = c0;
                    ++r;
                }
            }
        }
        // the faces of more than SMALL pixels, one at a time: all 64 lanes read the setup from the lane that made it
        unsigned long long todo = __ballot(n > SMALL);
        while (todo) {
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            Edge g[3];
            double gz[3];
            for (int i = 0; i < 3; ++i) {
                g[i].w00 = __shfl(e[i].w00, src);
                g[i].sc = __shfl(e[i].sc, src);
                g[i].sr = __shfl(e[i].sr, src);
                g[i].bias = __shfl(e[i].bias, src);
                gz[i] = __shfl(z[i], src);
            }
            const long long garea = __shfl(area, src);
            const int gc0 = __shfl(c0, src), gr0 = __shfl(r0, src), gbw = __shfl(bw, src), gn = __shfl(n, src);
            const unsigned gf = (unsigned)__shfl(f, src);
            for (int p = lane; p < gn; p += 64) {
                const int dr = p / gbw;
                cover(g, gz, garea, gf, gc0 + (p - dr * gbw), gr0 + dr, Z, W);
            }
        }
    }
}

__device__ __forceinline__ uint8_t to_byte(double x) {     // floor(x + 0.5) clamped to [0, 255]; a NaN gives 0
    return (uint8_t)fmin(fmax(floor(x + 0.5), 0.0), 255.0);
}

__global__ __launch_bounds__(NT) void raster_resolve_kernel(const unsigned long long* __restrict__ zbuf,
                                                            const float* __restrict__ xyz, const uint8_t* __restrict__ rgb,
                                                            const int* __restrict__ nvert, const int* __restrict__ faces,
                                                            const float* __restrict__ poses, const float* __restrict__ intrinsics,
                                                            int total, int B, int capv, int capf, int H, int W, int shade,
                                                            int background, uint8_t* __restrict__ frames, float* __restrict__ depth,
                                                            int* __restrict__ index, float* __restrict__ bary) {
    const int i = blockIdx.x * NT + threadIdx.x;           // total = K B H W < 2^31: the entry point checks it
    if (i >= total) return;
    const int hw = H * W, kb = i / hw, p = i - kb * hw, r = p / W, c = p - r * W, b = kb % B;
    const unsigned long long key = zbuf[i];
    const float* const Kb = intrinsics + (size_t)b * 16;
    Face F;
    bool hit = zbuf_hit(key, capf);
    if (hit)
        hit = face_setup(faces + ((size_t)b * capf + zbuf_row(key)) * 3, xyz + (size_t)b * capv * 3, clamped_count(nvert, b, capv),
                         poses + (size_t)kb * 16, Kb, 0.0, F);
    uint8_t out[3];
    zbuf_background(background, out);
    float wgt[3] = {__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("")};
    if (hit) {
        const long long w[3] = {edge_at(edge_of(F.v[1], F.v[2]), c, r), edge_at(edge_of(F.v[2], F.v[0]), c, r),
                                edge_at(edge_of(F.v[0], F.v[1]), c, r)};
        const double z[3] = {F.v[0].cam[2], F.v[1].cam[2], F.v[2].cam[2]};
        double q[3];
        const double s = weights(w, z, q);
        for (int j = 0; j < 3; ++j) {                      // weight j belongs to the face's j-th index as stored
            const float v = (float)(q[j] / s);
            wgt[0] = F.v[j].slot == 0 ? v : wgt[0];
            wgt[1] = F.v[j].slot == 1 ? v : wgt[1];
            wgt[2] = F.v[j].slot == 2 ? v : wgt[2];
        }
        if (shade == 0) {
            const uint8_t* const col = rgb + (size_t)b * capv * 3;
            for (int ch = 0; ch < 3; ++ch) {
                double cj[3];
                for (int j = 0; j < 3; ++j) cj[j] = (double)col[(size_t)F.v[j].row * 3 + ch];
                out[ch] = to_byte(((q[0] * cj[0] + q[1] * cj[1]) + q[2] * cj[2]) / s);
            }
        } else {
            double e1[3], e2[3];
            for (int a = 0; a < 3; ++a) {
                e1[a] = F.v[1].cam[a] - F.v[0].cam[a];
                e2[a] = F.v[2].cam[a] - F.v[0].cam[a];
            }
            const double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
            double d[3];                                   // the pixel's ray: the point of depth 1 on it
            on_ray(load_cam(Kb), (double)c, (double)r, 1.0, d);
            const double nd = (n[0] * d[0] + n[1] * d[1]) + n[2] * d[2];
            const double nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2], dd = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
            const double sh = fabs(nd) / sqrt(nn * dd);
            out[0] = out[1] = out[2] = isfinite(sh) ? to_byte(255.0 * sh) : (uint8_t)0;
        }
    }
    zbuf_store(i, hit, key, out, frames, depth, index);
    if (bary) {
        float* const w3 = bary + (size_t)i * 3;
        w3[0] = wgt[0];
        w3[1] = wgt[1];
        w3[2] = wgt[2];
    }
}

}  // namespace

extern "C" int cpn_raster_faces(const float* xyz, const int* nvert, const int* faces, const int* nface, const float* poses,
                                const float* intrinsics, int K, int B, int capv, int capf, int H, int W, int cull, double near,
                                unsigned long long* zbuf, void* stream) {
    CPN_REQUIRE(xyz && nvert && faces && nface && poses && intrinsics && zbuf, CPN_E_ARG, "cpn_raster_faces: null pointer");
    if (const int bad = check_image("cpn_raster_faces", K, B, H, W, MAX_SIDE)) return bad;
    const long long all_tiles = cpn_cdiv(capf, NT), tiles = all_tiles < TILES ? all_tiles : TILES;
    CPN_REQUIRE(capv >= 1 && capf >= 1 && (long long)K * B * all_tiles < (1LL << 31), CPN_E_SHAPE,
                "cpn_raster_faces: need capv, capf >= 1 and K B ceil(capf / 256) < 2^31 (got K %d, B %d, capv %d, capf %d)", K, B, capv,
                capf);
    CPN_REQUIRE((cull == 0 || cull == 1) && near > 0.0, CPN_E_ARG, "cpn_raster_faces: need cull 0 or 1 and near > 0 (got %d, %g)",
                cull, near);
    if (const int bad = zbuf_clear(zbuf, K, B, H, W, (hipStream_t)stream, "cpn_raster_faces")) return bad;
    hipLaunchKernelGGL(raster_faces_kernel, dim3((unsigned)(K * B * tiles)), dim3(NT), 0, (hipStream_t)stream, xyz, nvert, faces, nface,
                       poses, intrinsics, B, capv, capf, (int)tiles, H, W, cull, near, zbuf);
    CPN_LAUNCH_CHECK("cpn_raster_faces");
    return 0;
}

extern "C" int cpn_raster_resolve(const unsigned long long* zbuf, const float* xyz, const uint8_t* rgb, const int* nvert,
                                  const int* faces, const float* poses, const float* intrinsics, int K, int B, int capv, int capf,
                                  int H, int W, int shade, int background, uint8_t* frames, float* depth, int* index, float* bary,
                                  void* stream) {
    CPN_REQUIRE(zbuf && xyz && rgb && nvert && faces && poses && intrinsics && frames, CPN_E_ARG, "cpn_raster_resolve: null pointer");
    if (const int bad = check_image("cpn_raster_resolve", K, B, H, W, MAX_SIDE)) return bad;
    CPN_REQUIRE(capv >= 1 && capf >= 1, CPN_E_SHAPE, "cpn_raster_resolve: need capv, capf >= 1 (got %d, %d)", capv, capf);
    CPN_REQUIRE((shade == 0 || shade == 1) && background >= 0 && background <= 0xFFFFFF, CPN_E_ARG,
                "cpn_raster_resolve: need shade 0 or 1 and background = r | g << 8 | b << 16 (got %d, %d)", shade, background);
    const int total = K * B * H * W;
    hipLaunchKernelGGL(raster_resolve_kernel, dim3(cpn_cdiv(total, NT)), dim3(NT), 0, (hipStream_t)stream, zbuf, xyz, rgb, nvert, faces,
                       poses, intrinsics, total, B, capv, capf, H, W, shade, background, frames, depth, index, bary);
    CPN_LAUNCH_CHECK("cpn_raster_resolve");
    return 0;
}
