"""Float64 references of the first encoder layer's table-form backward (csrc/encode_bwd.hip, the level-3 scatter of
csrc/backward.hip) for tests/test_encode_bwd_ref.py (CPU) and tests/test_gpu_encode_bwd.py (GPU).  Helpers, not tests.

Nothing here looks at a kernel's output.  Index-deciding arithmetic follows the contract of the oracle's bilinear_taps: plain
IEEE fp32, one rounding per operation, in the order the kernels' headers state; every value is then formed in float64.
"""
import torch
import torch.nn.functional as F

from oracle.render_ref import gather_levels

PAD = 4                      # CPN_NODE_PAD: the zeros table reaches 4 nodes past the map on every side
TAB_LD = 832
WMAX = 2048                  # rows per work item of the bucketed table scatter
U32 = 2.0 ** -24             # unit roundoff of fp32, round to nearest
U16 = 2.0 ** -11             # unit roundoff of fp16

# (B, R, S, ray0, nrays) of test_encode_hidden_ragged_ranges
RAGGED = [
    (1, 1, 1, 0, 1),            # one row pair
    (1, 5, 3, 0, 5),            # neither a multiple of the 4-ray x 4-sample wave tile
    (2, 7, 9, 3, 9),            # a ray range that starts mid-group and crosses the batch boundary
    (3, 6, 33, 6, 12),          # all of batch element 1 and 2, none of 0
    (2, 17, 64, 30, 4),         # the tail of the last element
    (1, 130, 8, 1, 127),        # more than 8 workgroups' worth of wave tiles, odd ends
]
PILEUP = (1, 40, 64, 0, 40)     # 2560 rows per image and kind: more than WMAX


# ------------------------------------------------------------------------------------------------------------------
# geometry of the node tables
# ------------------------------------------------------------------------------------------------------------------
def table_dims(H, W, kind):
    """(rows, columns) of the border (kind 0) / zeros (kind 1) node table of an H x W image."""
    return H // 2 + 1 + 2 * PAD * kind, W // 2 + 1 + 2 * PAD * kind


def table_nodes(H, W):
    """Nodes per image, border table first (what cpn_encode_table_nodes returns)."""
    (h0, w0), (h1, w1) = table_dims(H, W, 0), table_dims(H, W, 1)
    return h0 * w0 + h1 * w1


def row_table(B, V, R, S, ray0, nrays):
    """Every row of the chunk [ray0, ray0 + nrays) in the header's order, row = (((b R + r - ray0) V + v) S + s) 2 + j:
    `img` the image it reads (j = 0: b V + v, j = 1: b V + (V-1-v)), `kind` = j (0: coordinate from pixel_val, border
    table; 1: from sec_grid, zeros table), `src` the index of its coordinate in the (N R S, 2) view of that tensor."""
    ray = torch.arange(ray0, ray0 + nrays).view(-1, 1, 1, 1)
    v = torch.arange(V).view(1, -1, 1, 1)
    s = torch.arange(S).view(1, 1, -1, 1)
    j = torch.arange(2).view(1, 1, 1, -1)
    ray, v, s, j = [t.reshape(-1) for t in torch.broadcast_tensors(ray, v, s, j)]
    b, r = ray // R, ray % R
    return {"img": b * V + torch.where(j == 0, v, V - 1 - v), "kind": j, "src": ((b * V + v) * R + r) * S + s,
            "b": b, "r": r, "v": v, "s": s}


def row_coords(rt, pixel_val, sec_grid):
    """(rows, 2) fp32 coordinate of every row of the table."""
    pv, sg = pixel_val.reshape(-1, 2)[rt["src"]], sec_grid.reshape(-1, 2)[rt["src"]]
    return torch.where(rt["kind"].view(-1, 1) == 0, pv, sg)


def node_taps_ref(g, kind, H, W):
    """The four table nodes (index inside the image's tables, border table first) and float64 weights of every sample.
    g (rows, 2) fp32, kind (rows,) 0 / 1.  node_cell() as fp32 elementwise ops in its order: scale, clamp to
    [-pad, M + pad], floor, min with M + pad - 1; the fractions are fp32 (tx - x0 is exact), the weights float64 products
    of them.  Tap k = (x0 + (k & 1), y0 + (k >> 1))."""
    assert g.dtype == torch.float32
    pad = (kind * PAD).float()
    cell, frac = [], []
    for axis, M in ((0, W // 2), (1, H // 2)):
        t = (g[:, axis] + 1.0) * (0.5 * M)
        t = torch.minimum(torch.maximum(t, -pad), M + pad)
        c0 = torch.minimum(torch.floor(t), M + pad - 1.0)
        frac.append((t - c0).double())
        cell.append((c0 + pad).long())
    nw = (W // 2 + 1 + 2 * PAD * kind).long()
    base = kind * (table_dims(H, W, 0)[0] * table_dims(H, W, 0)[1])
    nodes, wts = [], []
    for k in range(4):
        i, jy = k & 1, k >> 1
        nodes.append(base + (cell[1] + jy) * nw + cell[0] + i)
        wts.append((frac[0] if i else 1.0 - frac[0]) * (frac[1] if jy else 1.0 - frac[1]))
    return torch.stack(nodes, 1), torch.stack(wts, 1)


def scatter_tables_ref(d, img, nodes, wts, nimg, H, W):
    """dT[img * table_nodes + node_t] += a_t d[row] in float64 -> (want, S_abs, n): the sum, the same sum over |a_t d|,
    and the number of non-zero-weight taps every NODE receives (a term count per element: every channel of a node gets
    the same taps)."""
    per = table_nodes(H, W)
    d = d.double()
    want = torch.zeros(nimg * per, d.shape[1], dtype=torch.float64)
    s_abs = torch.zeros_like(want)
    n = torch.zeros(nimg * per, dtype=torch.float64)
    for k in range(4):
        idx = img * per + nodes[:, k]
        term = wts[:, k:k + 1] * d
        want.index_add_(0, idx, term)
        s_abs.index_add_(0, idx, term.abs())
        n.index_add_(0, idx, (wts[:, k] != 0).double())
    return want, s_abs, n


def scatter_gamma(n, rows_per_group):
    """gamma of |got - want| <= gamma S_abs for an element of cpn_scatter_rows_tables that receives n terms (a number or a
    tensor of per-element counts), from the kernel's operation count (first order in u = 2^-24, the standard bound: a
    term's relative error is u times the number of roundings it passes through).
      * the weight: fl(1 - fx), fl(1 - fy) and their product: 3 roundings (fx, fy themselves are exact and shared with
        the reference); the term du * w: 1 (0 if the compiler fuses it into the addition; du is an exact fp16 value);
      * additions: the terms of a node are added one by one into a register run (at most n - 1 roundings on any term's
        path), a run is added to the LDS tile when the cell position changes - a node is tap 0..3 of at most 4 cell
        positions of a work item - and a split tile's work items are added with atomics: at most 5 more per work item,
        of which a tile has at most rows_per_group // WMAX + 1 (rows_per_group: the rows of one image and kind).
    The cell and weights of the level-3 scatter (cpn_gather_rows_bwd_level3) are formed the same way and its tile sums
    are flushed with one atomic per (tile, row group): the same count covers it."""
    items = rows_per_group // WMAX + 1
    return (n + 4 + 5 * items) * U32


def elementwise_bound(s_abs, gamma, dmax):
    """gamma S_abs + 2^-20 max|d|: the floor covers weights formed from fp32 fractions where the float64 reference
    differs in the last bits of a coordinate (and keeps the bound meaningful where S_abs is tiny)."""
    return gamma * s_abs + 2.0 ** -20 * dmax


# ------------------------------------------------------------------------------------------------------------------
# grid_sample references
# ------------------------------------------------------------------------------------------------------------------
def lift_grid(grid, Hl, Wl):
    """A float64 grid whose PIXEL coordinates at an (Hl, Wl) level are the fp32 ones: ATen's fp32 grid_sample (and
    make_taps, the same expression) forms x = ((g + 1) * Wl - 1) / 2 in fp32, and that x decides the taps and is the
    weight.  Sampling float64 maps at the lifted grid keeps that contract and removes every other fp32 rounding."""
    assert grid.dtype == torch.float32
    out = []
    for axis, size in ((0, Wl), (1, Hl)):
        x = ((grid[..., axis] + 1.0) * float(size) - 1.0) / 2.0
        out.append((2.0 * x.double() + 1.0) / size - 1.0)
    return torch.stack(out, -1)


def node_grid(H, W, kind):
    """(1, nh, nw, 2) float64 sample coordinates g = (2 n - M) / M of every node of a table."""
    nh, nw = table_dims(H, W, kind)
    off = PAD * kind
    gx = (2.0 * (torch.arange(nw, dtype=torch.float64) - off) - W // 2) / (W // 2)
    gy = (2.0 * (torch.arange(nh, dtype=torch.float64) - off) - H // 2) / (H // 2)
    return torch.stack((gx.view(1, -1).expand(nh, nw), gy.view(-1, 1).expand(nh, nw)), -1).unsqueeze(0)


def node_features_ref(z0, z1, z2, H, W):
    """(N * table_nodes, 768) float64: the three coarse levels sampled at every node of both tables (border table:
    nodes 0..M, 'border'; zeros table: nodes -4..M+4, 'zeros'), image by image, border table first."""
    N = z0.shape[0]
    out = []
    for kind, padding in ((0, "border"), (1, "zeros")):
        grid = node_grid(H, W, kind).expand(N, -1, -1, -1)
        f = gather_levels([t.double() for t in (z0, z1, z2)], grid, padding)              # (N, nh, nw, 768)
        out.append(f.reshape(N, -1, 768))
    return torch.cat(out, 1).reshape(-1, 768)


def node_features_matrix(lvl, H, W):
    """(table_nodes, Hl * Wl) float64 weights of node_features_ref at one level, from one-hot maps: the adjoint's |.| sum
    and term counts come from it."""
    Hl, Wl = H >> (4 - lvl), W >> (4 - lvl)
    eye = torch.eye(Hl * Wl, dtype=torch.float64).view(1, Hl * Wl, Hl, Wl)
    out = []
    for kind, padding in ((0, "border"), (1, "zeros")):
        f = F.grid_sample(eye, node_grid(H, W, kind), mode="bilinear", padding_mode=padding, align_corners=False)
        out.append(f.reshape(Hl * Wl, -1).t())
    return torch.cat(out, 0)


def level_taps_ref(g, kind, Hl, Wl):
    """ATen's grid_sampler_2d taps of one level (align_corners=False; kind 0 'border', 1 'zeros') from fp32 pixel
    coordinates: texel index yc * Wl + xc (rows, 4), float64 weights (0 for taps outside the map)."""
    idx, frac = [], []
    for axis, size in ((0, Wl), (1, Hl)):
        x = ((g[:, axis] + 1.0) * float(size) - 1.0) / 2.0
        xb = torch.minimum(torch.maximum(x, torch.zeros_like(x)), torch.full_like(x, size - 1.0))
        x = torch.where(kind == 0, xb, torch.minimum(torch.maximum(x, torch.full_like(x, -2.0)), torch.full_like(x, size + 1.0)))
        x0 = torch.floor(x)
        frac.append((x - x0).double())
        idx.append(x0.long())
    tex, wts = [], []
    for k in range(4):
        i, jy = k & 1, k >> 1
        xi, yi = idx[0] + i, idx[1] + jy
        inside = (xi >= 0) & (xi < Wl) & (yi >= 0) & (yi < Hl)
        w = (frac[0] if i else 1.0 - frac[0]) * (frac[1] if jy else 1.0 - frac[1])
        tex.append(yi.clamp(0, Hl - 1) * Wl + xi.clamp(0, Wl - 1))
        wts.append(torch.where(inside, w, torch.zeros_like(w)))
    return torch.stack(tex, 1), torch.stack(wts, 1)


def _swap_views(t, B, V):
    return t.view(B, V, *t.shape[1:]).flip(1).reshape(t.shape)


def _rows(prim, sec, B, V, R, S):
    """(N, R, S, C) own / other samples -> (B R V S 2, C) in the header's row order."""
    C = prim.shape[-1]
    x = torch.stack((prim.view(B, V, R, S, C), sec.view(B, V, R, S, C)), dim=4)            # (B, V, R, S, 2, C)
    return x.permute(0, 2, 1, 3, 4, 5).reshape(B * R * V * S * 2, C)


def chunk_rows(x, B, V, R, S, ray0, nrays):
    """The rows of the ray range out of all B R V S 2 rows."""
    return x.reshape(B * R, V * S * 2, -1)[ray0:ray0 + nrays].reshape(nrays * V * S * 2, -1)


def gather_rows_ref(z, pixel_val, sec_grid, B, V, R, S, dtype=torch.float64):
    """(B R V S 2, sum C_l) gathered features of every row: gather_levels with 'border' at pixel_val on the own view and
    'zeros' at sec_grid on the swapped views.  float32: the maps and grids as they are (ATen's fp32 grid_sample, what
    test_encode_hidden_against_torch compares with).  float64: every level at its lifted grid, values in float64; autograd
    through it is the float64 adjoint."""
    if dtype == torch.float32:
        prim = gather_levels(z, pixel_val, "border")
        sec = gather_levels([_swap_views(t, B, V) for t in z], sec_grid, "zeros")
        return _rows(prim, sec, B, V, R, S)
    prim, sec = [], []
    for t in z:
        Hl, Wl = t.shape[-2:]
        prim.append(gather_levels([t.double()], lift_grid(pixel_val, Hl, Wl), "border"))
        sec.append(gather_levels([_swap_views(t.double(), B, V)], lift_grid(sec_grid, Hl, Wl), "zeros"))
    return _rows(torch.cat(prim, -1), torch.cat(sec, -1), B, V, R, S)


def encode_input_ref(z, pixel_val, sec_grid, pe6, B, V, R, S, dtype=torch.float64):
    """(B R V S 2, 835) input of the layer, [gather (832) | tanh(pt/5) (3)], in row order."""
    x = gather_rows_ref(z, pixel_val, sec_grid, B, V, R, S, dtype)
    pe5 = pe6.view(B, V, R, S, 2, 3).permute(0, 2, 1, 3, 4, 5).reshape(-1, 3).to(dtype)
    return torch.cat((x, pe5), -1)


def level3_bwd_ref(d, H, W, pixel_val, sec_grid, B, V, R, S, ray0, nrays):
    """grid_sample backward of the full-resolution level: d (chunk rows, 64) -> (N, 64, H, W) float64, by autograd through
    gather_levels([z3], grid, padding) over the row table (the gather is linear in z3: its value does not matter)."""
    z3 = torch.zeros(B * V, 64, H, W, dtype=torch.float64, requires_grad=True)
    x = chunk_rows(gather_rows_ref([z3], pixel_val, sec_grid, B, V, R, S), B, V, R, S, ray0, nrays)
    (x * d.double()).sum().backward()
    return z3.grad


# ------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------
RIM_T = (-4, -3.5, -2, -1, -0.25, 0, 0.5)            # the rim positions of test_encode_hidden_against_torch, in nodes


def node_coord(t, M):
    """Sample coordinate of node position t (in nodes of an axis with M cells): exact in fp32 for M a power of two."""
    return 2.0 * t / M - 1.0


def hostile_coords(H, W):
    """(K, 2) fp32 coordinates where taps go wrong: huge, +-1, on nodes, on texel centres of every level, the zero rim at
    both ends of both axes, footprints that straddle an 8 x 4-node tile corner (both tables) and an 8 x 4-pixel tile
    corner of the full-resolution level, and zero fractions (fx == 0 / fy == 0: taps redirected to the dummy cell)."""
    Mx, My = W // 2, H // 2
    c = [(1e10, -1e10), (-1e10, 1e10), (1e10, 1e10), (-1e10, 0.3), (0.2, 1e10),
         (1.0, 1.0), (-1.0, -1.0), (-1.0, 1.0), (1.0, -1.0), (0.0, 0.0)]
    for nx, ny in ((0, 0), (Mx, My), (8, 4), (7, 3), (Mx - 1, 1), (3, My)):              # exactly on nodes
        c.append((node_coord(nx, Mx), node_coord(ny, My)))
    for shift in (4, 3, 2, 0):                                                          # texel centres of every level
        Hl, Wl = H >> shift, W >> shift
        for tx, ty in ((0, 0), (Wl - 1, Hl - 1), (Wl // 2, 1)):
            c.append(((2 * tx + 1) / Wl - 1.0, (2 * ty + 1) / Hl - 1.0))
    for t in RIM_T:                                                                     # the zero rim, both axes, both ends
        c.append((node_coord(t, Mx), node_coord(My - t, My)))
        c.append((node_coord(Mx - t, Mx), node_coord(t, My)))
        c.append((node_coord(t, Mx), node_coord(t, My)))
        c.append((node_coord(Mx - t, Mx), node_coord(My - t, My)))
    for off in (0, PAD):                                                                # one row in four buckets
        for fx, fy in ((0.5, 0.5), (0.25, 0.75)):
            c.append((node_coord(7 + fx - off, Mx), node_coord(3 + fy - off, My)))
            c.append((node_coord(15 + fx - off, Mx), node_coord(7 + fy - off, My)))
    for px, py in ((7.5, 3.5), (15.25, 7.75), (7.5, 8.0), (8.0, 3.5)):                   # level-3 pixel tile corners / edges
        c.append(((2 * px + 1) / W - 1.0, (2 * py + 1) / H - 1.0))
    for nx, ny in ((5.0, 2.5), (5.5, 2.0), (8.0, 3.5), (7.5, 4.0)):                      # fx == 0 or fy == 0
        c.append((node_coord(nx, Mx), node_coord(ny, My)))
    return torch.tensor(c, dtype=torch.float32)


def random_coords(N, R, S, gen):
    """pixel_val in [-1.2, 1.2), sec_grid in [-1.5, 1.5): the ranges of the forward tests."""
    return (torch.rand(N, R, S, 2, generator=gen) * 2.4 - 1.2, torch.rand(N, R, S, 2, generator=gen) * 3 - 1.5)


def plant_hostile(pixel_val, sec_grid, H, W, gen):
    """Overwrite a random set of samples of both tensors with the hostile coordinates (as many as fit, at least one in
    four samples stays random)."""
    hc = hostile_coords(H, W)
    for t in (pixel_val, sec_grid):
        flat = t.view(-1, 2)
        k = min(len(hc), (3 * flat.shape[0]) // 4)
        where = torch.randperm(flat.shape[0], generator=gen)[:k]
        flat[where] = hc[torch.randperm(len(hc), generator=gen)[:k]]
    return pixel_val, sec_grid


def pileup_coords(H, W, gen):
    """Coordinates of the PILEUP shape (B = 1, V = 2, R = 40, S = 64; 2560 rows per image and kind):
      * pixel_val[0] (image 0, border table): every row inside the 8 x 4-node tile (1, 1), half of them in the single cell
        (10, 5), a quarter of those at one and the same point (a pile-up on one level-3 texel);
      * sec_grid[0] (image 1, zeros table): 1400 rows at +1e10 (all of their weight on the corner node), the rest in the
        last cell before it - more than WMAX rows in the rim tile that holds that corner;
      * pixel_val[1] / sec_grid[1]: random plus the hostile set."""
    R, S = PILEUP[1], PILEUP[2]
    Mx, My = W // 2, H // 2
    pv, sg = random_coords(2, R, S, gen)
    plant_hostile(pv[1:], sg[1:], H, W, gen)
    n = R * S
    u = torch.rand(n, 2, generator=gen)
    tx, ty = 8.0 + 6.98 * u[:, 0], 4.0 + 2.98 * u[:, 1]                        # cells (8..14, 4..6): inside the tile
    tx[: n // 2], ty[: n // 2] = 10.0 + 0.98 * u[: n // 2, 0] + 0.01, 5.0 + 0.98 * u[: n // 2, 1] + 0.01
    tx[: n // 8], ty[: n // 8] = 10.375, 5.625
    order = torch.randperm(n, generator=gen)
    pv[0] = torch.stack((node_coord(tx, Mx), node_coord(ty, My)), -1)[order].view(R, S, 2)
    u = torch.rand(n, 2, generator=gen)
    rim = torch.stack((node_coord(Mx + PAD - 1 + 0.01 + 0.98 * u[:, 0], Mx), node_coord(My + PAD - 1 + 0.01 + 0.98 * u[:, 1], My)), -1)
    rim[:1400] = 1e10
    sg[0] = rim[torch.randperm(n, generator=gen)].view(R, S, 2)
    return pv.float(), sg.float()


def make_maps(N, H, W, gen):
    """The four levels, NCHW fp32, rounded to fp16 first."""
    shp = [(256, H // 16, W // 16), (256, H // 8, W // 8), (256, H // 4, W // 4), (64, H, W)]
    return [torch.randn(N, *s, generator=gen).half().float() for s in shp]


def masked_grad(rows, cols, gen):
    """Random fp16 values with a random half of the entries zeroed: the ReLU-masked shape of the real gradient."""
    d = torch.randn(rows, cols, generator=gen)
    return (d * (torch.rand(rows, cols, generator=gen) < 0.5)).half()
