"""Yardsticks of coponerf_amd/mesh.py (csrc/mesh.hip) and the inputs of its tests: float64 numpy restatements of the three entry
points of include/coponerf_hip.h (round 18) in the kernels' own operation order (sums left to right from 0, one IEEE rounding per
operation, one rounding to fp32 at a store), and the analytic fixtures.  tests/test_mesh_ref.py holds them to independent forms
on the CPU.

The kernels run the same float64 sequence (the unit is built without contraction), so the GPU tests ask for the same fp32 bits.
That can only hold where no DECISION of the rule sits on its threshold: integrate therefore counts, per case, the decisions within
BAND = 1e-9 (relative to the sum of the absolute terms that form the compared value) of their threshold - Y_z <= 0, the pixel
rounding, the window test, s < -trunc, s / trunc against 1 and tsdf < 0 - and tests/test_mesh_ref.py asks every GPU fixture for
zero of them.
"""
import numpy as np

from tests import novel_views_ref as nr
from tests import point_cloud_ref as pr

BAND = 1e-9
DECISIONS = ("behind", "rounding", "window", "unseen", "clip", "sign")

# the twelve edges of a cell as (lower corner, upper corner), corner i = dx + 2 dy + 4 dz: the header's order
EDGES = ((0, 1), (2, 3), (4, 5), (6, 7), (0, 2), (1, 3), (4, 6), (5, 7), (0, 4), (1, 5), (2, 6), (3, 7))


def _positive(x):
    x = np.float32(x)
    return bool(np.isfinite(x) and x > 0)


def integrate(depth, valid, rgb, poses, intrinsics, origin, spacing, trunc, S, window, dims):
    """cpn_tsdf_integrate.  depth (K, B, h w) fp32, valid (K, B, h w) uint8, rgb (K, B, h w, 3) fp32, poses (K, B, 4, 4) fp32,
    intrinsics (B, 4, 4) fp32, origin / spacing (B, 3) fp32, trunc (B) fp32, dims = (Nx, Ny, Nz) -> dict of tsdf (B, Nz, Ny, Nx)
    fp32, weight uint8, colour (B, Nz, Ny, Nx, 3) fp32, near: DECISIONS -> the number of decisions inside the band, and steps:
    how many (voxel, view) visits ended at each step of the rule (the fixtures are asked to reach every one)."""
    depth = np.asarray(depth, dtype=np.float32)
    rgb = np.asarray(rgb, dtype=np.float32)
    K, B, R = depth.shape
    y0, x0, h, w = pr.window_of(S, window)
    Nx, Ny, Nz = dims
    vox = Nx * Ny * Nz
    tsdf = np.ones((B, vox), dtype=np.float32)
    weight = np.zeros((B, vox), dtype=np.uint8)
    colour = np.zeros((B, vox, 3), dtype=np.float32)
    near = dict.fromkeys(DECISIONS, 0)
    steps = dict.fromkeys(("behind", "outside", "bad_depth", "valid_byte", "unseen", "clipped", "inner"), 0)
    p = np.arange(vox)
    idx = (p % Nx, (p // Nx) % Ny, p // (Nx * Ny))
    P64 = np.asarray(poses, dtype=np.float32).astype(np.float64)
    for b in range(B):
        if not (_positive(trunc[b]) and all(_positive(s) for s in spacing[b])):
            continue                                                     # the empty volume
        tr = float(np.float32(trunc[b]))
        o, sp = np.asarray(origin[b], np.float32).astype(np.float64), np.asarray(spacing[b], np.float32).astype(np.float64)
        X = [o[a] + idx[a].astype(np.float64) * sp[a] for a in range(3)]
        fx, fy, cx, cy = pr.cam_of(intrinsics[b])
        total, col, n = np.zeros(vox), [np.zeros(vox) for _ in range(3)], np.zeros(vox, dtype=np.int64)
        for k in range(K):
            P = P64[k, b]
            with np.errstate(all="ignore"):
                d = [X[r] - P[r, 3] for r in range(3)]
                Y = [(P[0, j] * d[0] + P[1, j] * d[1]) + P[2, j] * d[2] for j in range(3)]
                My = np.abs(P[0, 2] * d[0]) + np.abs(P[1, 2] * d[1]) + np.abs(P[2, 2] * d[2])
                front = (Y[2] > 0.0) & np.isfinite(Y[0]) & np.isfinite(Y[1]) & np.isfinite(Y[2])
                near["behind"] += int((np.abs(Y[2]) <= BAND * My).sum())
                u, v = (fx * Y[0]) / Y[2] + cx, (fy * Y[1]) / Y[2] + cy
                uh, vh = u + 0.5, v + 0.5
                mu, mv = np.abs((fx * Y[0]) / Y[2]) + abs(cx) + 0.5, np.abs((fy * Y[1]) / Y[2]) + abs(cy) + 0.5
                near["rounding"] += int((front & ((np.abs(uh - np.rint(uh)) <= BAND * mu) | (np.abs(vh - np.rint(vh)) <= BAND * mv))).sum())
                near["window"] += int((front & ((np.abs(uh - x0) <= BAND * mu) | (np.abs(uh - (x0 + w)) <= BAND * mu) |
                                                (np.abs(vh - y0) <= BAND * mv) | (np.abs(vh - (y0 + h)) <= BAND * mv))).sum())
                c, r = np.floor(uh) - float(x0), np.floor(vh) - float(y0)
                inside = front & (c >= 0.0) & (c < float(w)) & (r >= 0.0) & (r < float(h))
                at = np.where(inside, r * w + c, 0.0).astype(np.int64)
                d32 = depth[k, b][at]
                good = inside & pr.valid(d32)
                lit = good & (valid[k, b][at] != 0)
                dd = np.where(lit, d32, 1.0).astype(np.float64)
                s = dd - Y[2]
                ms = np.abs(dd) + np.abs(Y[2]) + tr
                near["unseen"] += int((lit & (np.abs(s + tr) <= BAND * ms)).sum())
                upd = lit & ~(s < -tr)
                near["clip"] += int((upd & (np.abs(s - tr) <= BAND * ms)).sum())
                f = np.minimum(1.0, s / tr)
            steps["behind"] += int((~front).sum())
            steps["outside"] += int((front & ~inside).sum())
            steps["bad_depth"] += int((inside & ~good).sum())
            steps["valid_byte"] += int((good & ~lit).sum())
            steps["unseen"] += int((lit & ~upd).sum())
            steps["clipped"] += int((upd & (f == 1.0)).sum())
            steps["inner"] += int((upd & (f < 1.0)).sum())
            total = np.where(upd, total + np.where(upd, f, 0.0), total)
            for ch in range(3):
                col[ch] = np.where(upd, col[ch] + np.where(upd, rgb[k, b][at, ch].astype(np.float64), 0.0), col[ch])
            n += upd
        some = n > 0
        nn = np.where(some, n, 1).astype(np.float64)
        mean = total / nn
        near["sign"] += int((some & (np.abs(mean) <= BAND)).sum())
        tsdf[b] = np.where(some, mean, 1.0).astype(np.float32)
        weight[b] = n.astype(np.uint8)
        for ch in range(3):
            colour[b, :, ch] = np.where(some, col[ch] / nn, 0.0).astype(np.float32)
    return dict(tsdf=tsdf.reshape(B, Nz, Ny, Nx), weight=weight.reshape(B, Nz, Ny, Nx), colour=colour.reshape(B, Nz, Ny, Nx, 3),
                near=near, steps=steps)


def _corner(A, i):
    """Corner i = dx + 2 dy + 4 dz of every cell of the lattice array A (Nz, Ny, Nx, ...), the cells in (cz, cy, cx) order."""
    dx, dy, dz = i & 1, (i >> 1) & 1, i >> 2
    Nz, Ny, Nx = A.shape[:3]
    part = A[dz:Nz - 1 + dz, dy:Ny - 1 + dy, dx:Nx - 1 + dx]
    return part.reshape((-1,) + A.shape[3:])


def surface_vertices(tsdf, weight, colour, origin, spacing, min_weight=1):
    """cpn_surface_vertices -> (list of (n_b, 3) float32, list of (n_b, 3) uint8, nvert (B) int32, cell_vertex (B, cells) int32)."""
    tsdf, colour = np.asarray(tsdf, dtype=np.float32), np.asarray(colour, dtype=np.float32)
    B, Nz, Ny, Nx = tsdf.shape
    cells = (Nx - 1) * (Ny - 1) * (Nz - 1)
    out_xyz, out_rgb, nvert = [], [], np.zeros(B, dtype=np.int32)
    cell_vertex = np.full((B, cells), -1, dtype=np.int32)
    j = np.arange(cells)
    cell = (j % (Nx - 1), (j // (Nx - 1)) % (Ny - 1), j // ((Nx - 1) * (Ny - 1)))
    for b in range(B):
        f = [_corner(tsdf[b], i).astype(np.float64) for i in range(8)]
        C = [_corner(colour[b], i).astype(np.float64) for i in range(8)]
        with np.errstate(invalid="ignore"):
            ins = [x < 0.0 for x in f]
        seen = np.logical_and.reduce([_corner(weight[b], i).astype(np.int64) >= min_weight for i in range(8)])
        count = np.add.reduce([x.astype(np.int64) for x in ins])
        active = seen & (count != 0) & (count != 8)
        flags = active.astype(np.int64)
        row = np.cumsum(flags) - flags
        cell_vertex[b] = np.where(active, row, -1)
        nvert[b] = flags.sum()
        p, col, m = [np.zeros(cells) for _ in range(3)], [np.zeros(cells) for _ in range(3)], np.zeros(cells, dtype=np.int64)
        for e, (lo, hi) in enumerate(EDGES):
            axis = e // 4
            cross = active & (ins[lo] != ins[hi])
            with np.errstate(all="ignore"):
                t = np.where(cross, f[lo] / (f[lo] - f[hi]), 0.0)
                q = (float(lo & 1), float((lo >> 1) & 1), float(lo >> 2))
                for a in range(3):
                    p[a] = np.where(cross, p[a] + ((q[a] + t) if a == axis else q[a]), p[a])
                for ch in range(3):
                    col[ch] = np.where(cross, col[ch] + ((1.0 - t) * C[lo][:, ch] + t * C[hi][:, ch]), col[ch])
            m += cross
        src = np.flatnonzero(active)
        mm = m[src].astype(np.float64)
        o, sp = np.asarray(origin[b], np.float32).astype(np.float64), np.asarray(spacing[b], np.float32).astype(np.float64)
        xyz, rgb = np.empty((len(src), 3), dtype=np.float32), np.empty((len(src), 3), dtype=np.uint8)
        with np.errstate(all="ignore"):
            for a in range(3):
                xyz[:, a] = (o[a] + (cell[a][src].astype(np.float64) + p[a][src] / mm) * sp[a]).astype(np.float32)
                rgb[:, a] = nr.to_byte(((col[a][src] / mm).astype(np.float32) + np.float32(1)) * np.float32(127.5))
        out_xyz.append(xyz)
        out_rgb.append(rgb)
    return out_xyz, out_rgb, nvert, cell_vertex


def surface_faces(tsdf, cell_vertex):
    """cpn_surface_faces -> (list of (m_b, 3) int32, nface (B) int32).  Plain loops over the lattice edges in e = 3 voxel + axis
    order, the cells addressed by their coordinates."""
    tsdf = np.asarray(tsdf, dtype=np.float32)
    B, Nz, Ny, Nx = tsdf.shape
    N = (Nx, Ny, Nz)
    out, nface = [], np.zeros(B, dtype=np.int32)

    def cell_index(c):
        return (c[2] * (Ny - 1) + c[1]) * (Nx - 1) + c[0]

    for b in range(B):
        with np.errstate(invalid="ignore"):
            ins = tsdf[b] < 0                                            # (Nz, Ny, Nx)
        tris = []
        # only an edge whose ends differ can be selected: visit those, in ascending e
        cand = []
        for a in range(3):
            lo = [slice(None)] * 3
            hi = [slice(None)] * 3
            lo[2 - a], hi[2 - a] = slice(0, N[a] - 1), slice(1, N[a])
            iz, iy, ix = np.nonzero(ins[tuple(lo)] != ins[tuple(hi)])
            cand += [(3 * ((z * Ny + y) * Nx + x) + a, (x, y, z), a) for x, y, z in zip(ix.tolist(), iy.tolist(), iz.tolist())]
        for e, p, a in sorted(cand):
            ab, ac = (a + 1) % 3, (a + 2) % 3
            if not (p[ab] >= 1 and p[ab] + 1 < N[ab] and p[ac] >= 1 and p[ac] + 1 < N[ac]):
                continue
            v = []
            for db, dc in ((-1, -1), (0, -1), (0, 0), (-1, 0)):
                c = list(p)
                c[ab] += db
                c[ac] += dc
                v.append(int(cell_vertex[b, cell_index(c)]))
            if min(v) < 0:
                continue
            v00, v10, v11, v01 = v
            if ins[p[2], p[1], p[0]]:
                tris += [(v00, v10, v11), (v00, v11, v01)]
            else:
                tris += [(v00, v11, v10), (v00, v01, v11)]
        out.append(np.array(tris, dtype=np.int32).reshape(-1, 3))
        nface[b] = len(tris)
    return out, nface


def extract(tsdf, weight, colour, origin, spacing, min_weight=1):
    """Both stages -> dict of xyz, rgb, faces (lists per pair), nvert, nface, cell_vertex."""
    xyz, rgb, nvert, cell_vertex = surface_vertices(tsdf, weight, colour, origin, spacing, min_weight)
    faces, nface = surface_faces(tsdf, cell_vertex)
    return dict(xyz=xyz, rgb=rgb, faces=faces, nvert=nvert, nface=nface, cell_vertex=cell_vertex)


# ------------------------------------------------------------------------------------------------------- mesh properties
def edge_counts(faces):
    """{undirected edge: the number of triangles it lies in}."""
    counts = {}
    for tri in np.asarray(faces).tolist():
        for i in range(3):
            key = tuple(sorted((tri[i], tri[(i + 1) % 3])))
            counts[key] = counts.get(key, 0) + 1
    return counts


def signed_volume(xyz, faces):
    """The sum of the signed volumes of the tetrahedra (0, a, b, c): positive for outward normals."""
    x = np.asarray(xyz, dtype=np.float64)
    a, b, c = (x[np.asarray(faces)[:, i]] for i in range(3))
    return float((np.cross(a, b) * c).sum() / 6.0)


# ---------------------------------------------------------------------------------------------------------------- fixtures
_CACHE = {}


def _frozen(out):
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def _colours(shape, seed):
    """fp32 colours in [-1.1, 1.1], no NaN: a mean keeps its bits."""
    return np.random.default_rng(seed).uniform(-1.1, 1.1, size=shape).astype(np.float32)


MAIN_DIMS = (9, 7, 5)


def main_case():
    """Integrate, main case: K = 3, B = 2, S = 16, window (2, 3, 11, 12), dims (9, 7, 5).  The depth is point_cloud_ref's tilted
    plane and sphere, ray-cast in float64 and rounded to fp32, with NaN, +-inf, 0 and 10 planted; some valid bytes are 0.  The
    volumes start 0.1 in front of view 0, so part of them lies behind camera 2, which stands 0.3 (0.24) ahead; the two pairs
    differ in poses, intrinsics, origin, spacing and trunc."""
    if "main" in _CACHE:
        return _CACHE["main"]
    base = pr.scene(K=3, B=2, S=16, window=(2, 3, 11, 12))
    K, B, h, w = 3, 2, 11, 12
    depth = np.array(base["depth"]).reshape(K, B, h, w)
    depth[0, :, 1, :] = np.nan
    depth[1, :, 3, 2:7] = 0.0
    depth[1, :, 8, 5] = -np.inf
    depth[2, :, 4, :6] = 10.0
    depth[2, :, 9, 7] = np.inf
    valid = np.ones((K, B, h, w), dtype=np.uint8)
    valid[0, :, 6, 3:9] = 0
    valid[2, 1, 2:5, 8:] = 0
    valid[1, 0, 5, :] = 0
    out = dict(depth=depth.reshape(K, B, h * w), valid=valid.reshape(K, B, h * w), rgb=_colours((K, B, h * w, 3), 18),
               poses=np.array(base["poses"]), intrinsics=np.array(base["intrinsics"]), S=16, window=(2, 3, 11, 12), dims=MAIN_DIMS,
               origin=np.array([[-1.3, -1.1, 0.1], [-1.0, -0.9, 0.15]], dtype=np.float32),
               spacing=np.array([[0.31, 0.37, 1.1], [0.27, 0.33, 1.05]], dtype=np.float32),
               trunc=np.array([0.9, 1.3], dtype=np.float32))
    _CACHE["main"] = _frozen(out)
    return out


def degenerate_cases():
    """The main case with pair 1 made degenerate, three ways: trunc = 0, trunc = NaN, a non-positive spacing."""
    if "degenerate" in _CACHE:
        return _CACHE["degenerate"]
    base = main_case()
    out = []
    for trunc1, sy1 in ((0.0, 0.33), (np.nan, 0.33), (1.3, -0.33)):
        case = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in base.items()}
        case["trunc"][1] = trunc1
        case["spacing"][1, 1] = sy1
        out.append(_frozen(case))
    _CACHE["degenerate"] = out
    return out


def integrate_case(case):
    key = ("integrate", id(case))
    if key not in _CACHE:
        _CACHE[key] = (case, integrate(case["depth"], case["valid"], case["rgb"], case["poses"], case["intrinsics"], case["origin"],
                                       case["spacing"], case["trunc"], case["S"], case["window"], case["dims"]))
    return _CACHE[key][1]


def sphere_sdf(dims, origin, spacing, centre, radius):
    """(Nz, Ny, Nx) float64: the exact signed distance to the sphere at the lattice points."""
    Nx, Ny, Nz = dims
    z, y, x = np.meshgrid(np.arange(Nz), np.arange(Ny), np.arange(Nx), indexing="ij")
    X = [origin[a] + g * spacing[a] for a, g in enumerate((x, y, z))]
    return np.sqrt((X[0] - centre[0]) ** 2 + (X[1] - centre[1]) ** 2 + (X[2] - centre[2]) ** 2) - radius


EXTRACT_DIMS = (17, 13, 9)


def extract_case():
    """Extraction on given volumes, dims (17, 13, 9): 1 536 cells and 5 967 lattice edges, both past CPN_COMPACT_TILE = 1024.
    Pair 0 is a sphere (weights 2, one slab of 1 and one of 0, so min_weight = 2 opens it); pair 1 is hostile: random fp32 tsdf in
    [-1, 1] with exact 0, 1 and -1 planted, random weights in {0, 1, 2}, colours beyond [-1, 1] with a few NaN."""
    if "extract" in _CACHE:
        return _CACHE["extract"]
    Nx, Ny, Nz = EXTRACT_DIMS
    rng = np.random.default_rng(1805)
    origin = np.array([[-0.8, -0.6, 1.9], [0.3, -2.0, 0.5]], dtype=np.float32)
    spacing = np.array([[0.1, 0.1, 0.1], [0.07, 0.21, 0.13]], dtype=np.float32)
    tsdf = np.empty((2, Nz, Ny, Nx), dtype=np.float32)
    o64, s64 = origin.astype(np.float64), spacing.astype(np.float64)
    tsdf[0] = np.clip(sphere_sdf(EXTRACT_DIMS, o64[0], s64[0], (0.013, 0.021, 2.307), 0.36) / 0.3, -1.0, 1.0)
    tsdf[1] = rng.uniform(-1.0, 1.0, size=(Nz, Ny, Nx))
    flat = tsdf[1].reshape(-1)
    flat[rng.choice(flat.size, 240, replace=False)] = np.repeat(np.array([0.0, 1.0, -1.0, -0.0], dtype=np.float32), 60)
    weight = np.empty((2, Nz, Ny, Nx), dtype=np.uint8)
    weight[0] = 2
    weight[0, :, 3, :] = 1
    weight[0, 6, :, :5] = 0
    weight[1] = rng.choice(np.array([0, 1, 2], dtype=np.uint8), size=(Nz, Ny, Nx), p=(0.03, 0.07, 0.9))
    colour = pr.colours((2, Nz, Ny, Nx, 3), seed=18)
    out = dict(tsdf=tsdf, weight=weight, colour=colour, origin=origin, spacing=spacing, dims=EXTRACT_DIMS)
    _CACHE["extract"] = _frozen(out)
    return out


def extract_of(case, min_weight):
    key = ("extracted", id(case), min_weight)
    if key not in _CACHE:
        _CACHE[key] = (case, extract(case["tsdf"], case["weight"], case["colour"], case["origin"], case["spacing"], min_weight))
    return _CACHE[key][1]


CHAIN_DIMS = (24, 24, 24)
CHAIN_C, CHAIN_R = np.array([0.03, -0.02, 3.01]), 0.8
_CHAIN_MOVES = (((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)), ((0.0, 12.0, 0.0), (-0.62, 0.01, 0.07)), ((0.0, -11.0, 2.0), (0.58, -0.03, 0.05)),
                ((9.0, 0.0, -1.0), (0.02, 0.47, 0.04)))


def chain_case():
    """Chain: the analytic z-depth of a sphere from 4 cameras at S = 32 (NaN where a ray misses it), for a 24^3 volume over the
    box [-1, 1]^2 x [2, 4]."""
    if "chain" in _CACHE:
        return _CACHE["chain"]
    K, S = 4, 32
    # no round numbers: camera 0 is the identity and the lattice is rational, and no projection may fall on half a pixel
    intr = np.array([[[31.3, 0, 15.73, 0], [0, 32.9, 15.21, 0], [0, 0, 1, 0], [0, 0, 0, 1]]], dtype=np.float32)
    u, v = pr.pixel_grid(S, None)
    fx, fy, cx, cy = pr.cam_of(intr[0])
    ray = np.stack(((u - cx) / fx, (v - cy) / fy, np.ones_like(u)), axis=-1)
    poses = np.zeros((K, 1, 4, 4), dtype=np.float32)
    depth = np.empty((K, 1, S * S), dtype=np.float32)
    for k, (deg, t) in enumerate(_CHAIN_MOVES):
        poses[k, 0] = pr.rigid(deg, np.array(t))
        P = poses[k, 0].astype(np.float64)
        dirs, oc = ray @ P[:3, :3].T, P[:3, 3] - CHAIN_C
        qa, qb, qc = (dirs * dirs).sum(-1), 2.0 * (dirs @ oc), oc @ oc - CHAIN_R ** 2
        disc = qb * qb - 4.0 * qa * qc
        depth[k, 0] = np.where(disc > 0, (-qb - np.sqrt(np.abs(disc))) / (2.0 * qa), np.nan)        # lambda . (.., .., 1): the z-depth
    out = dict(depth=depth, valid=np.ones((K, 1, S * S), dtype=np.uint8), rgb=_colours((K, 1, S * S, 3), 81), poses=poses,
               intrinsics=intr, S=S, window=None, dims=CHAIN_DIMS, lo=np.array([[-1.0, -1.0, 2.0]], dtype=np.float32),
               hi=np.array([[1.0, 1.0, 4.0]], dtype=np.float32), trunc_voxels=3.0)
    # what coponerf_amd.mesh.integrate forms on the device, in fp32: (hi - lo) / (N - 1) and trunc_voxels . max
    out["origin"] = out["lo"].copy()
    out["spacing"] = ((out["hi"] - out["lo"]) / (np.array(CHAIN_DIMS, dtype=np.float32) - np.float32(1))[None]).astype(np.float32)
    out["trunc"] = (out["spacing"].max(axis=1) * np.float32(3.0)).astype(np.float32)
    _CACHE["chain"] = _frozen(out)
    return out


def gpu_fixtures():
    """name -> case of every integrate fixture the GPU tests run (each must report zero decisions in the band)."""
    cases = {"main": main_case(), "chain": chain_case()}
    for i, case in enumerate(degenerate_cases()):
        cases[f"degenerate{i}"] = case
    return cases
