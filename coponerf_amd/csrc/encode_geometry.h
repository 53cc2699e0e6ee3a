// Geometry of the first encoder layer's node tables and of the rows that read them, in ONE place for the forward
// (encode.hip, encode_fused.hip, encode_f32.hip) and the training backward (encode_bwd.hip, backward.hip): which table node
// a sample touches, which table row a node is, and which row of hid / of the gradient a (ray, view, sample, image) is.
// Plain arithmetic only, so that every translation unit can include it.
#pragma once
#include "common.h"
#include "taps.h"

namespace {

constexpr int PAD = CPN_NODE_PAD;         // zero rim of the 'zeros' table, in nodes (= level-0 texel pitch / 2)

// node-grid geometry of one image: the border table (kind 0) first, the zeros table (kind 1, with its rim) behind it
struct NodeGrid {
    int Mx, My;                           // W/2, H/2
    __host__ __device__ static int pad(int kind) { return kind ? PAD : 0; }
    __host__ __device__ int w(int kind) const { return kind ? Mx + 1 + 2 * PAD : Mx + 1; }
    __host__ __device__ int h(int kind) const { return kind ? My + 1 + 2 * PAD : My + 1; }
    __host__ __device__ long long border_nodes() const { return (long long)w(0) * h(0); }
    __host__ __device__ long long zeros_nodes() const { return (long long)w(1) * h(1); }
    __host__ __device__ long long nodes_per_image() const { return border_nodes() + zeros_nodes(); }
    // first table row of (image, kind)
    __host__ __device__ size_t table_base(int img, int kind) const {
        return (size_t)img * nodes_per_image() + (kind ? border_nodes() : 0);
    }
    // row of the cell at table coordinates (xi, yi) >= 0 inside its table, in the index width I of the call site
    template <class I = int>
    __host__ __device__ I cell(int kind, int xi, int yi) const { return (I)yi * w(kind) + xi; }
    // the same for node (nx, ny), counted from the image corner: the rim nodes of the zeros table are negative
    __host__ __device__ int node(int kind, int nx, int ny) const { return cell(kind, nx + pad(kind), ny + pad(kind)); }
    // node t <-> u = t / M <-> normalised g = 2u - 1 (exact when M is a power of two)
    __host__ __device__ float gx(int nx) const { return (float)(2 * nx - Mx) / (float)Mx; }
    __host__ __device__ float gy(int ny) const { return (float)(2 * ny - My) / (float)My; }
};

// table row -> the node it is
struct NodeId {
    int img, nx, ny;
    bool border;
    float gx, gy;                         // its normalised coordinate
};
__device__ __forceinline__ NodeId node_of(long long row, const NodeGrid ng) {
    NodeId o;
    const long long npi = ng.nodes_per_image();
    o.img = (int)(row / npi);
    long long rem = row - (long long)o.img * npi;
    o.border = rem < ng.border_nodes();
    if (!o.border) rem -= ng.border_nodes();
    const int nw = o.border ? ng.w(0) : ng.w(1), pad = o.border ? NodeGrid::pad(0) : NodeGrid::pad(1);
    o.ny = (int)(rem / nw) - pad;
    o.nx = (int)(rem % nw) - pad;
    o.gx = ng.gx(o.nx);
    o.gy = ng.gy(o.ny);
    return o;
}

// the cell of normalised coordinate g (grid_sample convention, [-1,1] = image) in table `kind`: table coordinates (>= 0) of
// its upper left node and the bilinear fractions towards the other three
struct NodeCell {
    int xi, yi;
    float fx, fy;
};
__device__ __forceinline__ NodeCell node_cell(float gx, float gy, int kind, const NodeGrid ng) {
    const int pad = NodeGrid::pad(kind);
    float tx = (gx + 1.0f) * (0.5f * (float)ng.Mx), ty = (gy + 1.0f) * (0.5f * (float)ng.My);
    // beyond the rim the function is constant (border: clamped; zeros: 0), and |g| can reach 1e10 (geometry.py:390-391)
    tx = fminf(fmaxf(tx, (float)-pad), (float)(ng.Mx + pad));
    ty = fminf(fmaxf(ty, (float)-pad), (float)(ng.My + pad));
    const int x0 = min((int)floorf(tx), ng.Mx + pad - 1), y0 = min((int)floorf(ty), ng.My + pad - 1);
    NodeCell c;
    c.fx = tx - (float)x0;
    c.fy = ty - (float)y0;
    c.xi = x0 + pad;
    c.yi = y0 + pad;
    return c;
}

// The rows that read image `img` = (b, vi) out of the ray range [rlo, rlo + per / S) of batch element b: idx in [0, per) is
// the own view (j = 0, sampled at pixel_val), [per, 2 per) the other view (j = 1, at sec_grid).  s_pow2: S is a power of
// two and rem / S is taken as rem >> s_shift.
struct RowRef {
    unsigned row;      // row of hid / of its gradient
    float2 g;          // normalised sample coordinate
    int j;
};
__device__ __forceinline__ RowRef row_of(int idx, int per, int S, bool s_pow2, int s_shift, int rlo, int b, int vi, int V,
                                         int R, int ray0, const float* __restrict__ pixel_val,
                                         const float* __restrict__ sec_grid) {
    RowRef o;
    o.j = idx >= per;
    const int rem = idx - o.j * per;
    const int rr = s_pow2 ? (rem >> s_shift) : (rem / S);
    const int sm = rem - rr * S;
    const int r = rlo + rr;
    const int v = o.j ? (V - 1 - vi) : vi;
    const size_t sidx = sample_index(b, V, v, R, r, S, sm);
    o.g = *reinterpret_cast<const float2*>((o.j ? sec_grid : pixel_val) + sidx * 2);
    o.row = ((((unsigned)(b * R + r - ray0)) * V + v) * S + sm) * 2 + o.j;
    return o;
}

}  // namespace
