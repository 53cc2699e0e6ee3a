// K rendered depth maps in, a coloured triangle mesh out (coponerf_amd/mesh.py): a truncated signed distance averaged per voxel
// over the views, and the zero level set of it by naive surface nets - one vertex per cell, so no triangle table.
//
//   tsdf_integrate_kernel     cpn_tsdf_integrate: one thread per voxel, the views in ascending order inside it.  x is fastest
//                             across a wave, so the K depth reads of neighbouring voxels fall on neighbouring pixels.
//   vertex_count_kernel /     cpn_surface_vertices: compact.h's two launches over a pair's cells in (cz, cy, cx) order; a
//   vertex_write_kernel       selected (active) cell writes its vertex, its colour and its row in cell_vertex.
//   face_count_kernel /       cpn_surface_faces: the same two launches over a pair's lattice edges e = 3 voxel + axis; a
//   face_write_kernel         selected edge writes the two triangles of the quad of its four cells.
//
// No atomics.  float64 from the fp32 inputs, one rounding per operation (-ffp-contract=off), sums left to right, one rounding
// to fp32 at a store: tests/mesh_ref.py restates it in numpy.  The camera and the rule of a valid depth are pinhole.h's.
#include "common.h"
#include "byte_pack.h"
#include "compact.h"
#include "pinhole.h"

#include <math.h>

namespace {

constexpr int NT = 256;
constexpr int TILE = CPN_COMPACT_TILE;
static_assert(COMPACT_NT == NT, "the compaction kernels run 256 threads");

struct Dims {
    int nx, ny, nz;
};

__device__ __forceinline__ bool positive(float v) { return v > 0.0f && v < __builtin_inff(); }     // finite and > 0

__global__ __launch_bounds__(NT) void tsdf_integrate_kernel(const float* __restrict__ depth, const uint8_t* __restrict__ valid,
                                                            const float* __restrict__ rgb, const float* __restrict__ poses,
                                                            const float* __restrict__ intrinsics, const float* __restrict__ origin,
                                                            const float* __restrict__ spacing, const float* __restrict__ trunc,
                                                            int total, int K, int B, int y0, int x0, int h, int w, Dims n,
                                                            float* __restrict__ tsdf, uint8_t* __restrict__ weight,
                                                            float* __restrict__ colour) {
    const int i = blockIdx.x * NT + threadIdx.x;           // total = B Nz Ny Nx < 2^31: the entry point checks it
    if (i >= total) return;
    const int vox = n.nx * n.ny * n.nz, b = i / vox, p = i - b * vox;
    const int iz = p / (n.nx * n.ny), q = p - iz * (n.nx * n.ny), iy = q / n.nx, ix = q - iy * n.nx;
    const float* const sp = spacing + (size_t)b * 3;
    const float* const og = origin + (size_t)b * 3;
    const float tr32 = trunc[b];
    double sum = 0.0, col[3] = {0.0, 0.0, 0.0};
    int cnt = 0;
    if (positive(tr32) && positive(sp[0]) && positive(sp[1]) && positive(sp[2])) {
        const double tr = (double)tr32;
        const double X[3] = {(double)og[0] + (double)ix * (double)sp[0], (double)og[1] + (double)iy * (double)sp[1],
                             (double)og[2] + (double)iz * (double)sp[2]};
        const Cam cam = load_cam(intrinsics + (size_t)b * 16);
        const int hw = h * w;
        for (int k = 0; k < K; ++k) {
            double Y[3], u, v;
            to_camera_centred(load_pose(poses + ((size_t)k * B + b) * 16), X, Y);
            if (!(Y[2] > 0.0 && finite3(Y[0], Y[1], Y[2]))) continue;
            project(cam, Y, u, v);
            const double c = floor(u + 0.5) - (double)x0, r = floor(v + 0.5) - (double)y0;
            if (!(c >= 0.0 && c < (double)w && r >= 0.0 && r < (double)h)) continue;          // outside the window, or NaN
            const size_t at = ((size_t)k * B + b) * hw + (size_t)((int)r * w + (int)c);
            const float d32 = depth[at];
            if (!depth_valid(d32) || valid[at] == 0) continue;
            const double s = (double)d32 - Y[2];
            if (s < -tr) continue;                         // behind the surface by more than the truncation: unseen
            sum += fmin(1.0, s / tr);
            for (int ch = 0; ch < 3; ++ch) col[ch] += (double)rgb[at * 3 + ch];
            ++cnt;
        }
    }
    weight[i] = (uint8_t)cnt;                              // cnt <= K <= 255
    tsdf[i] = cnt ? (float)(sum / (double)cnt) : 1.0f;
    for (int ch = 0; ch < 3; ++ch) colour[(size_t)i * 3 + ch] = cnt ? (float)(col[ch] / (double)cnt) : 0.0f;
}

// ---- surface nets.  Corner i = dx + 2 dy + 4 dz of cell (cx, cy, cz) is voxel (cx + dx, cy + dy, cz + dz).
// The twelve edges as (lower corner, upper corner): four x-edges, four y-edges, four z-edges, each group in (0,0), (1,0), (0,1),
// (1,1) order of the other two offsets (the lower axis first)
__device__ const unsigned char EDGE_LO[12] = {0, 2, 4, 6, 0, 1, 4, 5, 0, 1, 2, 3};
__device__ const unsigned char EDGE_HI[12] = {1, 3, 5, 7, 2, 3, 6, 7, 4, 5, 6, 7};

struct Cell {
    int cx, cy, cz;
};
__device__ __forceinline__ Cell cell_of(int j, Dims n) {
    const int mx = n.nx - 1, my = n.ny - 1;
    Cell c;
    c.cz = j / (mx * my);
    const int q = j - c.cz * (mx * my);
    c.cy = q / mx;
    c.cx = q - c.cy * mx;
    return c;
}
// voxel index of corner i of the cell, inside pair b's volume
__device__ __forceinline__ int corner_voxel(Cell c, int i, Dims n) {
    return ((c.cz + (i >> 2)) * n.ny + (c.cy + ((i >> 1) & 1))) * n.nx + (c.cx + (i & 1));
}

// observed (all eight weights >= min_weight) and neither all inside nor all outside
__device__ __forceinline__ bool cell_active(const float* __restrict__ T, const uint8_t* __restrict__ Wt, Cell c, Dims n,
                                            int min_weight) {
    int inside = 0;
    bool seen = true;
    for (int i = 0; i < 8; ++i) {
        const int v = corner_voxel(c, i, n);
        seen = seen && (int)Wt[v] >= min_weight;
        inside += T[v] < 0.0f ? 1 : 0;
    }
    return seen && inside != 0 && inside != 8;
}

__global__ __launch_bounds__(NT) void vertex_count_kernel(const float* __restrict__ tsdf, const uint8_t* __restrict__ weight,
                                                          Dims n, int cells, int min_weight, int* __restrict__ counts,
                                                          int* __restrict__ cell_vertex) {
    const int b = blockIdx.y;
    const size_t vox = (size_t)n.nx * n.ny * n.nz;
    const float* const T = tsdf + (size_t)b * vox;
    const uint8_t* const Wt = weight + (size_t)b * vox;
    for (int s = 0; s < COMPACT_SUB; ++s) {                // every element of cell_vertex is written: the second launch
        const int j = blockIdx.x * TILE + s * NT + threadIdx.x;                        // overwrites the active cells'
        if (j < cells) cell_vertex[(size_t)b * cells + j] = -1;
    }
    const int c = compact_tile_count(cells, [&](int j) { return cell_active(T, Wt, cell_of(j, n), n, min_weight); });
    if (threadIdx.x == 0) counts[(size_t)b * gridDim.x + blockIdx.x] = c;
}

__global__ __launch_bounds__(NT) void vertex_write_kernel(const float* __restrict__ tsdf, const uint8_t* __restrict__ weight,
                                                          const float* __restrict__ colour, const float* __restrict__ origin,
                                                          const float* __restrict__ spacing, Dims n, int cells, int min_weight,
                                                          int capv, const int* __restrict__ counts, float* __restrict__ vert_xyz,
                                                          uint8_t* __restrict__ vert_rgb, int* __restrict__ nvert,
                                                          int* __restrict__ cell_vertex) {
    const int b = blockIdx.y;
    const size_t vox = (size_t)n.nx * n.ny * n.nz;
    const float* const T = tsdf + (size_t)b * vox;
    const uint8_t* const Wt = weight + (size_t)b * vox;
    const float* const C = colour + (size_t)b * vox * 3;
    const int at = compact_tile_rows(
        counts + (size_t)b * gridDim.x, cells, [&](int j) { return cell_active(T, Wt, cell_of(j, n), n, min_weight); },
        [&](int j, int row) {
            cell_vertex[(size_t)b * cells + j] = row;
            if (row >= capv) return;                       // rows at and beyond the capacity are left untouched
            const Cell c = cell_of(j, n);
            int vx[8];
            double f[8];
            for (int i = 0; i < 8; ++i) {
                vx[i] = corner_voxel(c, i, n);
                f[i] = (double)T[vx[i]];
            }
            double p[3] = {0.0, 0.0, 0.0}, col[3] = {0.0, 0.0, 0.0};
            int m = 0;
            for (int e = 0; e < 12; ++e) {
                const int lo = EDGE_LO[e], hi = EDGE_HI[e], axis = e >> 2;
                if ((f[lo] < 0.0) == (f[hi] < 0.0)) continue;
                const double t = f[lo] / (f[lo] - f[hi]);
                const double q[3] = {(double)(lo & 1), (double)((lo >> 1) & 1), (double)(lo >> 2)};
                for (int a = 0; a < 3; ++a) p[a] += a == axis ? q[a] + t : q[a];
                for (int ch = 0; ch < 3; ++ch)
                    col[ch] += (1.0 - t) * (double)C[(size_t)vx[lo] * 3 + ch] + t * (double)C[(size_t)vx[hi] * 3 + ch];
                ++m;
            }
            const double cell[3] = {(double)c.cx, (double)c.cy, (double)c.cz};
            const size_t o = ((size_t)b * capv + (size_t)row) * 3;
            for (int a = 0; a < 3; ++a) {
                const double mean = p[a] / (double)m;      // m >= 3: an active cell has a sign change
                vert_xyz[o + a] = (float)((double)origin[b * 3 + a] + (cell[a] + mean) * (double)spacing[b * 3 + a]);
                vert_rgb[o + a] = to_byte(((float)(col[a] / (double)m) + 1.0f) * 127.5f);
            }
        });
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) nvert[b] = at;
}

// Lattice edge e = 3 voxel + axis a of pair b: with (a, b, c) cyclic, its cells (p_b - 1, p_c - 1), (p_b, p_c - 1), (p_b, p_c),
// (p_b - 1, p_c) at p_a.  Returns whether the edge is selected; v: the vertex rows of the four cells, lower: the lower end inside.
__device__ __forceinline__ bool edge_quad(const float* __restrict__ T, const int* __restrict__ CV, int e, Dims n, int (&v)[4],
                                          bool& lower) {
    const int voxel = e / 3, a = e - voxel * 3;
    const int N[3] = {n.nx, n.ny, n.nz};
    int p[3];
    p[2] = voxel / (n.nx * n.ny);
    const int q = voxel - p[2] * (n.nx * n.ny);
    p[1] = q / n.nx;
    p[0] = q - p[1] * n.nx;
    const int ab = (a + 1) % 3, ac = (a + 2) % 3;
    if (!(p[a] + 1 < N[a] && p[ab] >= 1 && p[ab] + 1 < N[ab] && p[ac] >= 1 && p[ac] + 1 < N[ac])) return false;
    const int step[3] = {1, n.nx, n.nx * n.ny};
    lower = T[voxel] < 0.0f;
    if (lower == (T[voxel + step[a]] < 0.0f)) return false;
    const int mx = n.nx - 1, my = n.ny - 1;
    const int cstep[3] = {1, mx, mx * my};
    const int c11 = (p[2] * my + p[1]) * mx + p[0];        // the cell whose corner 0 is the voxel
    v[0] = CV[c11 - cstep[ab] - cstep[ac]];
    v[1] = CV[c11 - cstep[ac]];
    v[2] = CV[c11];
    v[3] = CV[c11 - cstep[ab]];
    return v[0] >= 0 && v[1] >= 0 && v[2] >= 0 && v[3] >= 0;
}

__global__ __launch_bounds__(NT) void face_count_kernel(const float* __restrict__ tsdf, const int* __restrict__ cell_vertex, Dims n,
                                                        int cells, int edges, int* __restrict__ counts) {
    const int b = blockIdx.y;
    const float* const T = tsdf + (size_t)b * n.nx * n.ny * n.nz;
    const int* const CV = cell_vertex + (size_t)b * cells;
    const int c = compact_tile_count(edges, [&](int e) {
        int v[4];
        bool lower;
        return edge_quad(T, CV, e, n, v, lower);
    });
    if (threadIdx.x == 0) counts[(size_t)b * gridDim.x + blockIdx.x] = c;
}

__global__ __launch_bounds__(NT) void face_write_kernel(const float* __restrict__ tsdf, const int* __restrict__ cell_vertex, Dims n,
                                                        int cells, int edges, int capf, const int* __restrict__ counts,
                                                        int* __restrict__ faces, int* __restrict__ nface) {
    const int b = blockIdx.y;
    const float* const T = tsdf + (size_t)b * n.nx * n.ny * n.nz;
    const int* const CV = cell_vertex + (size_t)b * cells;
    const int at = compact_tile_rows(
        counts + (size_t)b * gridDim.x, edges,
        [&](int e) {
            int v[4];
            bool lower;
            return edge_quad(T, CV, e, n, v, lower);
        },
        [&](int e, int row) {
            int v[4];
            bool lower;
            edge_quad(T, CV, e, n, v, lower);
            // (v00, v10, v11), (v00, v11, v01) with the lower end inside, the other winding otherwise
            const int tri[2][3] = {{v[0], lower ? v[1] : v[2], lower ? v[2] : v[1]}, {v[0], lower ? v[2] : v[3], lower ? v[3] : v[2]}};
            for (int t = 0; t < 2; ++t) {
                const long long f = 2LL * row + t;
                if (f >= capf) continue;                   // rows at and beyond the capacity are left untouched
                int* const o = faces + ((size_t)b * capf + (size_t)f) * 3;
                o[0] = tri[t][0];
                o[1] = tri[t][1];
                o[2] = tri[t][2];
            }
        });
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) nface[b] = (int)min(2LL * at, 2147483647LL);
}

long long voxels_of(int Nx, int Ny, int Nz) { return (long long)Nx * Ny * Nz; }
long long cells_of(int Nx, int Ny, int Nz) { return (long long)(Nx - 1) * (Ny - 1) * (Nz - 1); }

// the lattice of the extraction: B <= 65535 (the pairs are the grid's second dimension), 3 B voxels < 2^31 (and so B cells)
bool lattice_ok(int B, int Nx, int Ny, int Nz) {
    return B >= 1 && B <= 65535 && Nx >= 2 && Ny >= 2 && Nz >= 2 && 3 * (double)B * Nx * Ny * Nz < 2147483648.0;
}

int check_lattice(const char* who, int B, int Nx, int Ny, int Nz) {
    CPN_REQUIRE(lattice_ok(B, Nx, Ny, Nz), CPN_E_SHAPE,
                "%s: need 1 <= B <= 65535, Nx, Ny, Nz >= 2 and 3 B Nx Ny Nz < 2^31 (got B %d, dims %d x %d x %d)", who, B, Nx, Ny, Nz);
    return 0;
}

}  // namespace

extern "C" int cpn_tsdf_integrate(const float* depth, const uint8_t* valid, const float* rgb, const float* poses,
                                  const float* intrinsics, const float* origin, const float* spacing, const float* trunc, int K,
                                  int B, int S, int y0, int x0, int h, int w, int Nx, int Ny, int Nz, float* tsdf, uint8_t* weight,
                                  float* colour, void* stream) {
    CPN_REQUIRE(depth && valid && rgb && poses && intrinsics && origin && spacing && trunc && tsdf && weight && colour, CPN_E_ARG,
                "cpn_tsdf_integrate: null pointer");
    CPN_REQUIRE(K >= 1 && K <= 255 && B >= 1 && h >= 1 && w >= 1 && (long long)K * B * h * w < (1LL << 31), CPN_E_SHAPE,
                "cpn_tsdf_integrate: need 1 <= K <= 255 views, B, h, w >= 1 and K B h w < 2^31 (got K %d, B %d, h %d, w %d)", K, B, h,
                w);
    CPN_REQUIRE(S >= 1 && y0 >= 0 && x0 >= 0 && y0 <= S - h && x0 <= S - w, CPN_E_SHAPE,
                "cpn_tsdf_integrate: the window (%d, %d, %d, %d) does not lie in the %d x %d grid", y0, x0, h, w, S, S);
    CPN_REQUIRE(Nx >= 2 && Ny >= 2 && Nz >= 2 && (double)B * Nx * Ny * Nz < 2147483648.0, CPN_E_SHAPE,
                "cpn_tsdf_integrate: need Nx, Ny, Nz >= 2 and B Nx Ny Nz < 2^31 (got B %d, dims %d x %d x %d)", B, Nx, Ny, Nz);
    const int total = (int)(B * voxels_of(Nx, Ny, Nz));
    hipLaunchKernelGGL(tsdf_integrate_kernel, dim3(cpn_cdiv(total, NT)), dim3(NT), 0, (hipStream_t)stream, depth, valid, rgb, poses,
                       intrinsics, origin, spacing, trunc, total, K, B, y0, x0, h, w, Dims{Nx, Ny, Nz}, tsdf, weight, colour);
    CPN_LAUNCH_CHECK("cpn_tsdf_integrate");
    return 0;
}

extern "C" int cpn_surface_vertices_scratch(int B, int Nx, int Ny, int Nz) {
    if (!lattice_ok(B, Nx, Ny, Nz)) return 0;
    return (int)(B * (long long)cpn_cdiv(cells_of(Nx, Ny, Nz), TILE));
}

extern "C" int cpn_surface_vertices(const float* tsdf, const uint8_t* weight, const float* colour, const float* origin,
                                    const float* spacing, int B, int Nx, int Ny, int Nz, int min_weight, int capv, int* scratch,
                                    float* vert_xyz, uint8_t* vert_rgb, int* nvert, int* cell_vertex, void* stream) {
    CPN_REQUIRE(tsdf && weight && colour && origin && spacing && scratch && vert_xyz && vert_rgb && nvert && cell_vertex, CPN_E_ARG,
                "cpn_surface_vertices: null pointer");
    if (const int bad = check_lattice("cpn_surface_vertices", B, Nx, Ny, Nz)) return bad;
    CPN_REQUIRE(min_weight >= 1 && min_weight <= 255 && capv >= 1, CPN_E_ARG,
                "cpn_surface_vertices: need 1 <= min_weight <= 255 and capv >= 1 (got %d, %d)", min_weight, capv);
    const int cells = (int)cells_of(Nx, Ny, Nz);
    const Dims n{Nx, Ny, Nz};
    const dim3 grid(cpn_cdiv(cells, TILE), B);
    hipLaunchKernelGGL(vertex_count_kernel, grid, dim3(NT), 0, (hipStream_t)stream, tsdf, weight, n, cells, min_weight, scratch,
                       cell_vertex);
    CPN_LAUNCH_CHECK("cpn_surface_vertices (count)");
    hipLaunchKernelGGL(vertex_write_kernel, grid, dim3(NT), 0, (hipStream_t)stream, tsdf, weight, colour, origin, spacing, n, cells,
                       min_weight, capv, (const int*)scratch, vert_xyz, vert_rgb, nvert, cell_vertex);
    CPN_LAUNCH_CHECK("cpn_surface_vertices (write)");
    return 0;
}

extern "C" int cpn_surface_faces_scratch(int B, int Nx, int Ny, int Nz) {
    if (!lattice_ok(B, Nx, Ny, Nz)) return 0;
    return (int)(B * (long long)cpn_cdiv(3 * voxels_of(Nx, Ny, Nz), TILE));
}

extern "C" int cpn_surface_faces(const float* tsdf, const int* cell_vertex, int B, int Nx, int Ny, int Nz, int capf, int* scratch,
                                 int* faces, int* nface, void* stream) {
    CPN_REQUIRE(tsdf && cell_vertex && scratch && faces && nface, CPN_E_ARG, "cpn_surface_faces: null pointer");
    if (const int bad = check_lattice("cpn_surface_faces", B, Nx, Ny, Nz)) return bad;
    CPN_REQUIRE(capf >= 1, CPN_E_ARG, "cpn_surface_faces: need capf >= 1 (got %d)", capf);
    const int cells = (int)cells_of(Nx, Ny, Nz), edges = (int)(3 * voxels_of(Nx, Ny, Nz));
    const Dims n{Nx, Ny, Nz};
    const dim3 grid(cpn_cdiv(edges, TILE), B);
    hipLaunchKernelGGL(face_count_kernel, grid, dim3(NT), 0, (hipStream_t)stream, tsdf, cell_vertex, n, cells, edges, scratch);
    CPN_LAUNCH_CHECK("cpn_surface_faces (count)");
    hipLaunchKernelGGL(face_write_kernel, grid, dim3(NT), 0, (hipStream_t)stream, tsdf, cell_vertex, n, cells, edges, capf,
                       (const int*)scratch, faces, nface);
    CPN_LAUNCH_CHECK("cpn_surface_faces (write)");
    return 0;
}
