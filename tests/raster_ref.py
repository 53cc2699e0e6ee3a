"""numpy restatements of csrc/raster.hip's two entry points, in the operation order include/coponerf_hip.h fixes, and the cases of
tests/test_gpu_raster.py.  Pinned on the CPU by tests/test_raster_ref.py against a painter's implementation and closed forms.

Every result is an integer or a bit pattern.  Coverage is int64 arithmetic on the snapped vertices: it has no band at all.
numpy's float64 element-wise operations round once each, as the kernel's do with contraction off, so the comparison on the GPU is
exact; `band` marks the floating-point decisions within BAND of a threshold - Y_z of near, 256 u + 0.5 and 256 v + 0.5 of an
integer (the snap's floor, and with it the 2^29 limit), a colour + 0.5 of an integer (the byte roundings) - and
tests/test_raster_ref.py holds every case to none.
"""
import numpy as np

from tests import splat_ref as sr

BAND = 1e-9
EMPTY = np.uint64(2 ** 64 - 1)
LIM = 2.0 ** 29
NEAR = 1e-3
SMALL = 64                                                             # CPN_RASTER_SMALL: the cases straddle it
NAN_BITS = 0x7FC00000
WINDOW = 8                                                             # boxes up to WINDOW x WINDOW pixels are walked together


# ------------------------------------------------------------------------------------------------------------ restatements
def _area(X, Y, a, b, c):
    return (X[:, b] - X[:, a]) * (Y[:, c] - Y[:, a]) - (Y[:, b] - Y[:, a]) * (X[:, c] - X[:, a])


def setup(xyz32, nv, tri, pose32, intr32, near):
    """The header's DRAWABLE test and canonical order for the m faces `tri` (m, 3) int32 of one pair in one camera ->
    dict of ok (m), front (m), area (m) int64, X, Y (m, 3) int64, cam (m, 3, 3) float64 (vertex, axis), row, slot (m, 3), band (m)."""
    with np.errstate(invalid="ignore"):                                # rows beyond nvert may hold any bits
        xyz = np.asarray(xyz32, dtype=np.float32).astype(np.float64)
    P, Km = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (pose32, intr32))
    tri = np.asarray(tri).astype(np.int64).reshape(-1, 3)
    m = tri.shape[0]
    R, t = P[:3, :3], P[:3, 3]
    fx, fy, cx, cy = Km[0, 0], Km[1, 1], Km[0, 2], Km[1, 2]
    camera_ok = bool(np.isfinite(P[:3]).all() and np.isfinite([fx, fy, cx, cy]).all())
    inside = ((tri >= 0) & (tri < nv)).all(axis=1)
    rows = np.where(inside[:, None], tri, 0) if nv > 0 else np.zeros_like(tri)
    with np.errstate(all="ignore"):
        Xv = xyz[rows] if nv > 0 else np.full((m, 3, 3), np.nan)       # (m, vertex, axis)
        ok = inside & camera_ok & np.isfinite(Xv).all(axis=(1, 2))
        d = Xv - t
        cam = np.stack([(R[0, j] * d[..., 0] + R[1, j] * d[..., 1]) + R[2, j] * d[..., 2] for j in range(3)], axis=-1)
        z = cam[..., 2]
        band = ok & (np.abs(z - near) < BAND).any(axis=1)
        ok = ok & ((z >= near) & (z > 0.0) & np.isfinite(z.astype(np.float32))).all(axis=1)
        su = 256.0 * ((fx * cam[..., 0]) / z + cx) + 0.5
        sv = 256.0 * ((fy * cam[..., 1]) / z + cy) + 0.5
        fu, fv = np.floor(su), np.floor(sv)
        band |= ok & ((np.abs(su - np.rint(su)) < BAND) | (np.abs(sv - np.rint(sv)) < BAND)).any(axis=1)
        ok = ok & ((np.abs(fu) < LIM) & (np.abs(fv) < LIM)).all(axis=1)                 # a NaN fails
    X = np.where(ok[:, None], fu, 0).astype(np.int64)
    Y = np.where(ok[:, None], fv, 0).astype(np.int64)
    stored = _area(X, Y, 0, 1, 2)
    ok = ok & (stored != 0)
    front = stored < 0
    order = np.argsort(rows, axis=1, kind="stable")                    # ascending row; equal rows are equal points: area 0
    take = lambda a: np.take_along_axis(a, order, axis=1)
    Xs, Ys = take(X), take(Y)
    flip = _area(Xs, Ys, 0, 1, 2) < 0
    order = np.where(flip[:, None], order[:, [0, 2, 1]], order)
    Xs, Ys = take(X), take(Y)
    area = _area(Xs, Ys, 0, 1, 2)
    assert (area[ok] > 0).all()
    cams = np.take_along_axis(cam, order[:, :, None], axis=1)
    return dict(ok=ok, front=front, area=area, X=Xs, Y=Ys, cam=cams, row=take(rows), slot=order, band=band)


def edges(s):
    """The three edge functions of every face of a setup, as (w00, sc, sr, bias), each (m, 3): w_i at pixel (c, r) is
    w00 + c sc + r sr, the edge opposite vertex i: (1 -> 2), (2 -> 0), (0 -> 1)."""
    a, b = [1, 2, 0], [2, 0, 1]
    dx, dy = s["X"][:, b] - s["X"][:, a], s["Y"][:, b] - s["Y"][:, a]
    w00 = dy * s["X"][:, a] - dx * s["Y"][:, a]
    owns = (dy < 0) | ((dy == 0) & (dx > 0))                             # the top-left rule
    return w00, -256 * dy, 256 * dx, np.where(owns, 0, 1).astype(np.int64)


def _depth(w, z, area):
    """(q (.., 3), s (..), z32 (..)) of the edge values w (.., 3) int64, the vertices' camera z (.., 3) and the doubled area."""
    with np.errstate(all="ignore"):
        q = w.astype(np.float64) / z
        s = (q[..., 0] + q[..., 1]) + q[..., 2]
        return q, s, (area.astype(np.float64) / s).astype(np.float32)


def boxes(s, H, W):
    """The bounding boxes clipped to the image -> (c0, r0, bw, bh), bw = bh = 0 where the face is not drawn."""
    c0 = np.maximum((s["X"].min(axis=1) + 255) >> 8, 0)
    r0 = np.maximum((s["Y"].min(axis=1) + 255) >> 8, 0)
    c1 = np.minimum(s["X"].max(axis=1) >> 8, W - 1)
    r1 = np.minimum(s["Y"].max(axis=1) >> 8, H - 1)
    drawn = s["ok"] & (c1 >= c0) & (r1 >= r0)
    return c0, r0, np.where(drawn, c1 - c0 + 1, 0), np.where(drawn, r1 - r0 + 1, 0)


def covered(s, H, W, select):
    """Every (face, pixel) that the fill rule covers, of the faces `select` (bool (m)) -> (face (n), pixel r W + c (n), z32 (n))."""
    c0, r0, bw, bh = boxes(s, H, W)
    w00, sc, sr, bias = edges(s)
    todo = np.flatnonzero(select & (bw > 0))
    small = todo[(bw[todo] <= WINDOW) & (bh[todo] <= WINDOW)]
    groups = [(small, WINDOW, WINDOW)] if small.size else []
    groups += [(np.array([f]), int(bw[f]), int(bh[f])) for f in todo[(bw[todo] > WINDOW) | (bh[todo] > WINDOW)]]
    out = [(np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32))]
    for f, tw, th in groups:
        dr, dc = np.meshgrid(np.arange(th), np.arange(tw), indexing="ij")
        c = c0[f, None, None] + dc[None]
        r = r0[f, None, None] + dr[None]
        w = w00[f, None, None, :] + c[..., None] * sc[f, None, None, :] + r[..., None] * sr[f, None, None, :]
        hit = ((w - bias[f, None, None, :]) >= 0).all(axis=-1) & (dc[None] < bw[f, None, None]) & (dr[None] < bh[f, None, None])
        fi, yi, xi = np.nonzero(hit)
        _, _, z32 = _depth(w[fi, yi, xi], s["cam"][f[fi], :, 2], s["area"][f[fi]])
        out.append((f[fi], r[fi, yi, xi] * W + c[fi, yi, xi], z32))
    return tuple(np.concatenate(x) for x in zip(*out))


def _counts(n, b, cap):
    return min(max(int(n[b]), 0), cap)


def raster_faces(mesh, poses, intrinsics, H, W, cull=0, near=NEAR):
    """cpn_raster_faces -> (zbuf (K, B, H, W) uint64, band (K, B, capf) bool, times (K, B, H, W) int64: how many faces cover
    each pixel, before the depth test)."""
    K, B = poses.shape[0], poses.shape[1]
    capv, capf = mesh["xyz"].shape[1], mesh["faces"].shape[1]
    zbuf = np.full((K, B, H * W), EMPTY, dtype=np.uint64)
    times = np.zeros((K, B, H * W), dtype=np.int64)
    band = np.zeros((K, B, capf), dtype=bool)
    for k in range(K):
        for b in range(B):
            nf = _counts(mesh["nface"], b, capf)
            s = setup(mesh["xyz"][b], _counts(mesh["nvert"], b, capv), mesh["faces"][b, :nf], poses[k, b], intrinsics[b], near)
            band[k, b, :nf] = s["band"]
            face, pixel, z32 = covered(s, H, W, s["ok"] & (s["front"] | (cull == 0)))
            key = (z32.view(np.uint32).astype(np.uint64) << np.uint64(32)) | face.astype(np.uint64)
            np.minimum.at(zbuf[k, b], pixel, key)
            np.add.at(times[k, b], pixel, 1)
    return zbuf.reshape(K, B, H, W), band, times.reshape(K, B, H, W)


def _byte(x):
    """(floor(x + 0.5) clamped to [0, 255] as uint8, NaN -> 0; whether x + 0.5 lies within BAND of an integer)."""
    with np.errstate(all="ignore"):
        y = x + 0.5
        return np.fmin(np.fmax(np.floor(y), 0.0), 255.0).astype(np.uint8), np.abs(y - np.rint(y)) < BAND


def resolve(zbuf, mesh, poses, intrinsics, shade=0, background=(0, 0, 0)):
    """cpn_raster_resolve -> dict of frames (K, B, H, W, 3) uint8, bits (K, B, H, W) uint32 of the depth (NAN_BITS where empty:
    compare with isnan there), index (K, B, H, W) int32, bary (K, B, H, W, 3) float32 (NaN where empty: compare the bits
    elsewhere), band (K, B, H, W) bool: a byte rounding of the pixel within BAND of its threshold."""
    K, B, H, W = zbuf.shape
    capv, capf = mesh["xyz"].shape[1], mesh["faces"].shape[1]
    frames = np.empty((K, B, H, W, 3), dtype=np.uint8)
    frames[...] = np.asarray(background, dtype=np.uint8)
    bits = np.full((K, B, H, W), NAN_BITS, dtype=np.uint32)
    index = np.full((K, B, H, W), -1, dtype=np.int32)
    bary = np.full((K, B, H, W, 3), np.nan, dtype=np.float32)
    band = np.zeros((K, B, H, W), dtype=bool)
    for k in range(K):
        for b in range(B):
            key = zbuf[k, b]
            low = (key & np.uint64(0xFFFFFFFF)).astype(np.int64)
            r, c = np.nonzero((key != EMPTY) & (low < capf))
            f = low[r, c]
            s = setup(mesh["xyz"][b], _counts(mesh["nvert"], b, capv), mesh["faces"][b][f], poses[k, b], intrinsics[b], 0.0)
            keep = s["ok"]
            r, c, f = r[keep], c[keep], f[keep]
            s = {name: a[keep] for name, a in s.items()}
            w00, sc, sr, _ = edges(s)
            q, tot, _ = _depth(w00 + c[:, None] * sc + r[:, None] * sr, s["cam"][:, :, 2], s["area"])
            index[k, b, r, c] = f
            bits[k, b, r, c] = (key[r, c] >> np.uint64(32)).astype(np.uint32)
            with np.errstate(all="ignore"):
                wgt = (q / tot[:, None]).astype(np.float32)
                stored = np.empty_like(wgt)
                np.put_along_axis(stored, s["slot"], wgt, axis=1)       # weight j goes where vertex j stands in the face's row
                bary[k, b, r, c] = stored
                if shade == 0:
                    col = mesh["rgb"][b].astype(np.float64)[s["row"]]   # (n, vertex, channel)
                    x = ((q[:, 0, None] * col[:, 0] + q[:, 1, None] * col[:, 1]) + q[:, 2, None] * col[:, 2]) / tot[:, None]
                    byte, near_half = _byte(x)
                    frames[k, b, r, c] = byte
                    band[k, b, r, c] = near_half.any(axis=1)
                else:
                    Km = intrinsics[b].astype(np.float64)
                    e1, e2 = s["cam"][:, 1] - s["cam"][:, 0], s["cam"][:, 2] - s["cam"][:, 0]
                    n = np.stack((e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                                  e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]), axis=1)
                    d = np.stack(((c.astype(np.float64) - Km[0, 2]) / Km[0, 0], (r.astype(np.float64) - Km[1, 2]) / Km[1, 1],
                                  np.ones(c.shape)), axis=1)
                    dot = lambda a, b_: (a[:, 0] * b_[:, 0] + a[:, 1] * b_[:, 1]) + a[:, 2] * b_[:, 2]
                    sh = np.abs(dot(n, d)) / np.sqrt(dot(n, n) * dot(d, d))
                    byte, near_half = _byte(255.0 * sh)
                    fine = np.isfinite(sh)
                    frames[k, b, r, c] = np.where(fine, byte, 0)[:, None]
                    band[k, b, r, c] = fine & near_half
    return dict(frames=frames, bits=bits, index=index, bary=bary, band=band)


_CACHE = {}


def draw(case, cull=0, shade=0, background=(0, 0, 0)):
    """The whole of a case -> dict of zbuf, times, frames, bits, index, bary, band (the faces' any() or the pixels' any())."""
    key = (id(case), cull, shade, tuple(background))
    if key not in _CACHE:
        zkey = (id(case), cull)
        if zkey not in _CACHE:
            _CACHE[zkey] = (case, raster_faces(case, case["poses"], case["intrinsics"], case["H"], case["W"], cull))
        zbuf, band, times = _CACHE[zkey][1]
        out = resolve(zbuf, case, case["poses"], case["intrinsics"], shade, background)
        out.update(zbuf=zbuf, times=times, band=bool(band.any() or out["band"].any()))
        _CACHE[key] = (case, out)
    return _CACHE[key][1]


def same(got, want):
    """The GPU's zbuf (uint64), index, bits (uint32), bary (float32) and frames against draw()'s, exactly."""
    assert np.array_equal(got["zbuf"], want["zbuf"])
    assert np.array_equal(got["index"], want["index"])
    empty = want["index"] < 0
    assert np.isnan(got["bits"].view(np.float32)[empty]).all() and np.isnan(got["bary"][empty]).all()
    assert np.array_equal(got["bits"][~empty], want["bits"][~empty])
    assert np.array_equal(got["bary"][~empty].view(np.uint32), want["bary"][~empty].view(np.uint32))
    assert np.array_equal(got["frames"], want["frames"])


# ------------------------------------------------------------------------------------------------------------------- cases
rigid, intrinsics_of, place = sr.rigid, sr.intrinsics_of, sr.place
EYE = np.eye(4, dtype=np.float32)


def _frozen(case):
    for a in case.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return case


def _mesh(verts, rgb, faces, nvert=None, nface=None, **more):
    """One pair per entry of the lists -> the arrays of a Mesh, the capacities the longest of each."""
    B, capv, capf = len(verts), max(len(v) for v in verts), max(len(f) for f in faces)
    xyz = np.zeros((B, capv, 3), dtype=np.float32)
    col = np.zeros((B, capv, 3), dtype=np.uint8)
    tri = np.zeros((B, capf, 3), dtype=np.int32)
    for b in range(B):
        xyz[b, :len(verts[b])], col[b, :len(verts[b])], tri[b, :len(faces[b])] = verts[b], rgb[b], faces[b]
    nvert = np.array([len(v) for v in verts] if nvert is None else nvert, dtype=np.int32)
    nface = np.array([len(f) for f in faces] if nface is None else nface, dtype=np.int32)
    return dict(xyz=xyz, rgb=col, faces=tri, nvert=nvert, nface=nface, B=B, capv=capv, capf=capf, **more)


def grid_faces(ny, nx):
    """The 2 (ny - 1)(nx - 1) triangles of a grid of ny x nx vertices (row-major), diagonals alternating."""
    out = []
    for j in range(ny - 1):
        for i in range(nx - 1):
            a, b, c, d = j * nx + i, j * nx + i + 1, (j + 1) * nx + i + 1, (j + 1) * nx + i
            out += [(a, b, c), (a, c, d)] if (i + j) % 2 == 0 else [(a, b, d), (b, c, d)]
    return np.array(out, dtype=np.int32)


SHEET_H, SHEET_W = 40, 48


def sheet_vertices(rng, pose, intr, H=SHEET_H, W=SHEET_W, n=12):
    """A jittered n x n height field whose projection in the camera reaches 2 pixels beyond the H x W image on every side."""
    gv, gu = np.meshgrid(np.linspace(-2.0, H + 1.0, n), np.linspace(-2.0, W + 1.0, n), indexing="ij")
    inner = np.zeros((n, n), dtype=bool)
    inner[1:-1, 1:-1] = True
    u = gu + np.where(inner, rng.uniform(-1.2, 1.2, size=(n, n)), 0.0) + 0.013
    v = gv + np.where(inner, rng.uniform(-1.0, 1.0, size=(n, n)), 0.0) + 0.017
    return place(pose, intr, u.reshape(-1), v.reshape(-1), rng.uniform(2.0, 3.0, size=n * n))


def sheet_case():
    """The 242-face sheet alone in the identity camera, 48 x 40: every pixel is covered by exactly one face."""
    if "sheet" in _CACHE:
        return _CACHE["sheet"]
    rng = np.random.default_rng(1901)
    intr = intrinsics_of(52.0, 47.0, 23.4, 19.7)[None]
    verts = sheet_vertices(rng, EYE, intr[0])
    case = _mesh([verts], [rng.integers(0, 256, size=(144, 3), dtype=np.uint8)], [grid_faces(12, 12)], poses=EYE[None, None],
                 intrinsics=intr, H=SHEET_H, W=SHEET_W, K=1)
    _CACHE["sheet"] = _frozen(case)
    return case


def lattice_case():
    """The edge-sharing rule: a 9 x 11 grid of vertices that project EXACTLY onto integer and half-integer pixel positions
    (identity camera, z = 1, fx = fy = 4, x and y multiples of 1/8), 160 faces over a 20 x 16 image: pixel centres lie on
    shared edges (the horizontal, vertical and diagonal ones) and on vertices."""
    if "lattice" in _CACHE:
        return _CACHE["lattice"]
    rng = np.random.default_rng(1902)
    intr = intrinsics_of(4.0, 4.0, 0.0, 0.0)[None]
    gy, gx = np.meshgrid(np.arange(9) * 2.5 - 1.0, np.arange(11) * 2.5 - 1.5, indexing="ij")      # pixels: multiples of 1/2
    verts = np.stack((gx.reshape(-1) / 4.0, gy.reshape(-1) / 4.0, np.ones(99)), axis=1).astype(np.float32)
    case = _mesh([verts], [rng.integers(0, 256, size=(99, 3), dtype=np.uint8)], [grid_faces(9, 11)], poses=EYE[None, None],
                 intrinsics=intr, H=16, W=20, K=1, pixel_uv=np.stack((gx.reshape(-1), gy.reshape(-1)), axis=1))
    _CACHE["lattice"] = _frozen(case)
    return case


def reindexed(case, how):
    """The case with every face's indices rotated (how = 1, 2) or reversed (how = -1): same surface, other storage."""
    out = {k: v for k, v in case.items()}
    out["faces"] = np.ascontiguousarray(case["faces"][:, :, ::-1] if how < 0 else np.roll(case["faces"], how, axis=2))
    return _frozen(out)


MAIN_CAMERAS = (((0, 0, 0), (0, 0, 0)), ((2.0, -5.0, 1.0), (0.20, -0.05, 0.10)), ((-3.0, 6.0, -2.0), (-0.15, 0.10, 2.2)))


def main_case():
    """H x W = 40 x 48, K = 3, B = 2, non-square intrinsics.  Camera 0 is the identity, camera 1 turns and moves a little,
    camera 2 stands 2.2 ahead: the sheet (z in [2, 3]) is partly behind it and partly nearer than near or astride it.
    Pair 0's faces, in order: the 242 of the sheet; 24 loose triangles of 3 .. 25 pixels, partly outside the image, nearer than
    the sheet or behind it; 6 behind camera 0; 6 with one vertex behind camera 0 and two in front (astride near: dropped
    whole); then seven that would show at depth 1.1 (rows case["hostile"] ..): one with an index >= nvert, one with an index
    >= capv, one with a negative index, one with a NaN vertex, one with an infinite vertex, one of zero area (an index
    twice), one with all its vertices beyond nvert; then rows beyond nface that would cover the whole image at depth 0.5.
    Pair 1 has nface = 0, and after its sheet such rows too."""
    if "main" in _CACHE:
        return _CACHE["main"]
    rng = np.random.default_rng(1903)
    H, W, K, B = SHEET_H, SHEET_W, 3, 2
    intr = np.stack((intrinsics_of(52.0, 47.0, 23.4, 19.7), intrinsics_of(45.0, 51.0, 24.6, 20.2)))
    poses = np.stack([np.stack([rigid(deg, np.array(t) * (1.0 - 0.1 * b)) for b in range(B)]) for deg, t in MAIN_CAMERAS])
    verts = [sheet_vertices(rng, EYE, intr[0])]
    faces = [grid_faces(12, 12)]

    def loose(n, cu, cv, size, depth):
        base = sum(len(v) for v in verts)
        ang = rng.uniform(0, 2 * np.pi, size=(n, 1)) + np.array([0.0, 2.1, 4.2])[None] + rng.uniform(-0.4, 0.4, size=(n, 3))
        u, v = cu[:, None] + size[:, None] * np.cos(ang) + 0.011, cv[:, None] + size[:, None] * np.sin(ang) + 0.007
        verts.append(place(EYE, intr[0], u.reshape(-1), v.reshape(-1), np.broadcast_to(depth, (n, 3)).reshape(-1).astype(np.float64)))
        tri = base + np.arange(3 * n, dtype=np.int32).reshape(n, 3)
        tri[1::2] = tri[1::2, ::-1]                                    # both windings
        faces.append(tri)

    loose(24, rng.uniform(-3, W + 3, 24), rng.uniform(-3, H + 3, 24), rng.uniform(1.5, 4.0, 24), rng.uniform(1.2, 4.0, size=(24, 3)))
    loose(6, rng.uniform(5, W - 5, 6), rng.uniform(5, H - 5, 6), rng.uniform(2.0, 4.0, 6), -rng.uniform(0.5, 2.0, size=(6, 3)))
    astride = rng.uniform(1.0, 2.0, size=(6, 3))
    astride[:, 1] = -rng.uniform(0.2, 1.0, size=6)
    loose(6, rng.uniform(5, W - 5, 6), rng.uniform(5, H - 5, 6), rng.uniform(2.0, 4.0, 6), astride)
    n_ok = sum(len(f) for f in faces)
    big = place(EYE, intr[0], np.array([-300.0, 400.0, 0.0]), np.array([-300.0, 0.0, 400.0]), 0.5 * np.ones(3))
    n_big = sum(len(v) for v in verts)
    verts.append(big)                                                  # rows below nvert: only nface keeps them from showing
    loose(7, rng.uniform(8, W - 8, 7), rng.uniform(8, H - 8, 7), rng.uniform(2.0, 4.0, 7), 1.1 * np.ones((7, 3)))
    xyz0 = np.concatenate(verts)
    nvert0 = len(xyz0) - 3                                             # the last loose triangle's vertices lie beyond nvert
    tri0 = np.concatenate(faces)
    hostile = tri0[n_ok:].copy()                                       # seven faces that would show at depth 1.1
    assert len(hostile) == 7 and (hostile[:6] < nvert0).all() and (hostile[6] >= nvert0).all()
    hostile[0, 1] = nvert0 + 1                                         # a row of xyz, but beyond nvert
    hostile[1, 2] = 1 << 20                                            # beyond capv
    hostile[2, 0] = -1
    xyz0[hostile[3, 1], 2] = np.nan
    xyz0[hostile[4, 0], 0] = np.inf
    hostile[5, 2] = hostile[5, 0]                                      # two indices the same: zero area
    tri0[n_ok:] = hostile
    nface0 = len(tri0)
    cover = np.array([[0, 1, 2], [0, 2, 1]], dtype=np.int32)
    tri0 = np.concatenate((tri0, n_big + cover, n_big + cover))
    xyz1 = np.concatenate((sheet_vertices(rng, EYE, intr[1]), big))
    tri1 = np.concatenate((grid_faces(12, 12), 144 + cover))
    case = _mesh([xyz0, xyz1], [rng.integers(0, 256, size=(len(xyz0), 3), dtype=np.uint8),
                                rng.integers(0, 256, size=(len(xyz1), 3), dtype=np.uint8)], [tri0, tri1],
                 nvert=[nvert0, len(xyz1)], nface=[nface0, 0], poses=poses, intrinsics=intr, H=H, W=W, K=K, hostile=n_ok)
    _CACHE["main"] = _frozen(case)
    return case


MIXED_BIG = (37, 150)                                                  # the rows of the two image-filling faces


def mixed_case():
    """Large and small in one wave: a 64 x 64 image in the identity camera, 208 faces.  Rows 37 and 150 are the two halves of a
    quad at depth 3 that covers the whole image; the others are small right triangles, alternately at depth 2 and 4, whose
    clipped boxes hold 1, 63 (7 x 9), 64 (8 x 8), 65 (5 x 13) and a few other numbers of pixels: CPN_RASTER_SMALL and its
    two neighbours, in the same waves as the large faces."""
    if "mixed" in _CACHE:
        return _CACHE["mixed"]
    rng = np.random.default_rng(1904)
    H = W = 64
    intr = intrinsics_of(61.0, 67.0, 31.3, 32.8)[None]
    shapes = [(1, 1), (7, 9), (8, 8), (5, 13), (13, 5), (3, 4), (9, 7), (2, 2), (16, 4), (4, 16), (11, 6), (1, 64)]
    verts, faces, want_boxes = [], [], []
    for f in range(208):
        base = 3 * f
        if f in MIXED_BIG:
            u, v = (np.array([-5.3, 70.4, 70.4]), np.array([-4.6, -4.6, 69.7])) if f == MIXED_BIG[0] else \
                (np.array([-5.3, 70.4, -5.3]), np.array([-4.6, 69.7, 69.7]))
            depth = np.array([3.0, 3.1, 2.9]) if f == MIXED_BIG[0] else np.array([3.0, 2.9, 2.8])
            want_boxes.append(H * W)
        else:
            bw, bh = shapes[f % len(shapes)]
            c0, r0 = int(rng.integers(0, W - bw + 1)), int(rng.integers(0, H - bh + 1))
            u = np.array([c0 - 0.31, c0 + bw - 1 + 0.33, c0 - 0.31])
            v = np.array([r0 - 0.29, r0 - 0.29, r0 + bh - 1 + 0.32])
            depth = (2.0 if f % 2 == 0 else 4.0) + rng.uniform(-0.2, 0.2, size=3)
            want_boxes.append(bw * bh)
        verts.append(place(EYE, intr[0], u, v, depth))
        faces.append(base + np.roll(np.arange(3, dtype=np.int32), f % 3))
    case = _mesh([np.concatenate(verts)], [rng.integers(0, 256, size=(624, 3), dtype=np.uint8)], [np.array(faces, dtype=np.int32)],
                 poses=EYE[None, None], intrinsics=intr, H=H, W=W, K=1, boxes=np.array(want_boxes))
    _CACHE["mixed"] = _frozen(case)
    return case


def wide_case():
    """70 400 faces in a 96 x 96 image in one turned camera: 275 tiles of 256 faces, more than the CPN_RASTER_TILES = 256
    workgroups a pair gets, so the first 19 workgroups take a second tile - the rows above 65 535, which must win pixels.  Most
    faces cover a pixel or two, a third of them lie off the image."""
    if "wide" in _CACHE:
        return _CACHE["wide"]
    rng = np.random.default_rng(1905)
    n, H, W = 70400, 96, 96
    intr = intrinsics_of(101.0, 97.0, 47.2, 48.7)[None]
    pose = rigid((4.0, -7.0, 3.0), (0.3, -0.2, 0.1))
    cu, cv, size = rng.uniform(-12, W + 12, n), rng.uniform(-12, H + 12, n), rng.uniform(0.4, 1.8, n)
    ang = rng.uniform(0, 2 * np.pi, size=(n, 1)) + np.array([0.0, 2.1, 4.2])[None] + rng.uniform(-0.4, 0.4, size=(n, 3))
    u, v = cu[:, None] + size[:, None] * np.cos(ang), cv[:, None] + size[:, None] * np.sin(ang)
    depth = rng.uniform(1.0, 6.0, size=(n, 1)) + rng.uniform(-0.05, 0.05, size=(n, 3))
    xyz = place(pose, intr[0], u.reshape(-1), v.reshape(-1), depth.reshape(-1))
    case = _mesh([xyz], [rng.integers(0, 256, size=(3 * n, 3), dtype=np.uint8)], [np.arange(3 * n, dtype=np.int32).reshape(n, 3)],
                 poses=pose[None, None], intrinsics=intr, H=H, W=W, K=1)
    _CACHE["wide"] = _frozen(case)
    return case


PILE_N = 4096
PILE_A, PILE_B = (3, 2), (5, 6)                                        # (column, row) of the two pixels
PILE_SPLIT = PILE_N // 2


def pile_case():
    """An 8 x 8 image, the identity camera.  Faces 0 .. 4095: coincident triangles (each with vertex rows of its own, its
    indices rotated by its row) around the centre of pixel PILE_A, all vertices at z = 2.5: ONE fp32 depth, face 0 must win.
    Faces 4096 .. 8191 around pixel PILE_B: the first half at z = 2.5 + 2^-22 (the next float), the second half at z = 2.5:
    the nearer bit pattern wins over the lower rows, and of its faces the lowest, 4096 + 2048."""
    if "pile" in _CACHE:
        return _CACHE["pile"]
    rng = np.random.default_rng(1906)
    intr = intrinsics_of(9.0, 8.0, 3.6, 3.3)[None]
    du, dv = np.array([-0.41, 0.43, -0.05]), np.array([-0.37, -0.22, 0.45])
    verts, faces = [], []
    for f in range(2 * PILE_N):
        (c, r), z = (PILE_A, 2.5) if f < PILE_N else (PILE_B, 2.5 + 2.0 ** -22 if f < PILE_N + PILE_SPLIT else 2.5)
        verts.append(place(EYE, intr[0], c + du, r + dv, z * np.ones(3)))
        faces.append(3 * f + np.roll(np.arange(3, dtype=np.int32), f % 3))
    case = _mesh([np.concatenate(verts)], [rng.integers(0, 256, size=(6 * PILE_N, 3), dtype=np.uint8)],
                 [np.array(faces, dtype=np.int32)], poses=EYE[None, None], intrinsics=intr, H=8, W=8, K=1)
    _CACHE["pile"] = _frozen(case)
    return case


SPHERE_C, SPHERE_R = (0.013, 0.021, 2.307), 0.36


def sphere_case():
    """A closed sphere: surface nets (tests/mesh_ref.py's extract) of the exact signed distance on mesh_ref's 17 x 13 x 9 lattice,
    every voxel observed, seen from outside by three cameras in a 40 x 40 image."""
    if "sphere" in _CACHE:
        return _CACHE["sphere"]
    from tests import mesh_ref as mr
    rng = np.random.default_rng(1907)
    dims = mr.EXTRACT_DIMS
    origin, spacing = np.array([[-0.8, -0.6, 1.9]], dtype=np.float32), np.array([[0.1, 0.1, 0.1]], dtype=np.float32)
    tsdf = np.clip(mr.sphere_sdf(dims, origin[0].astype(np.float64), spacing[0].astype(np.float64), SPHERE_C, SPHERE_R) / 0.3,
                   -1.0, 1.0).astype(np.float32)[None]
    weight = np.full(tsdf.shape, 2, dtype=np.uint8)
    colour = rng.uniform(-1, 1, size=tsdf.shape + (3,)).astype(np.float32)
    got = mr.extract(tsdf, weight, colour, origin, spacing)
    moves = (((0, 0, 0), (0, 0, 0)), ((0.0, 25.0, 0.0), (-0.95, 0.02, 0.25)), ((-20.0, -8.0, 3.0), (0.3, -0.8, 0.1)))
    poses = np.stack([rigid(deg, np.array(t))[None] for deg, t in moves])
    case = _mesh([got["xyz"][0]], [got["rgb"][0]], [got["faces"][0]], poses=poses, intrinsics=intrinsics_of(58.0, 55.0, 19.4, 20.3)[None],
                 H=40, W=40, K=3)
    _CACHE["sphere"] = _frozen(case)
    return case


def near_side(case, k):
    """The case in its camera k alone, with only the faces that wind towards that camera: the others' rows are made (0, 0, 0),
    faces of zero area, so that every face keeps its row."""
    key = ("near side", id(case), k)
    if key not in _CACHE:
        s = setup(case["xyz"][0], int(case["nvert"][0]), case["faces"][0], case["poses"][k, 0], case["intrinsics"][0], NEAR)
        out = {name: v for name, v in case.items()}
        out["faces"] = np.where((s["ok"] & s["front"])[None, :, None], case["faces"], 0).astype(np.int32)
        out.update(poses=case["poses"][k:k + 1], K=1, kept=int((s["ok"] & s["front"]).sum()))
        _CACHE[key] = (case, _frozen(out))
    return _CACHE[key][1]


def tilted_case():
    """One tilted, vertex-coloured triangle in the identity camera, 24 x 20: two of its vertices project exactly onto pixel
    centres ((3, 2) and (19, 5): x = u z / fx with fx = 8, cx = cy = 0 and z a power of two), the third between them."""
    if "tilted" in _CACHE:
        return _CACHE["tilted"]
    intr = intrinsics_of(8.0, 8.0, 0.0, 0.0)[None]
    verts = np.array([[3.0 * 2.0 / 8.0, 2.0 * 2.0 / 8.0, 2.0], [19.0 * 4.0 / 8.0, 5.0 * 4.0 / 8.0, 4.0], [1.07, 2.31, 1.3]], dtype=np.float32)
    rgb = np.array([[250, 10, 60], [20, 240, 130], [90, 70, 255]], dtype=np.uint8)
    case = _mesh([verts], [rgb], [np.array([[0, 1, 2]], dtype=np.int32)], poses=EYE[None, None], intrinsics=intr, H=20, W=24, K=1,
                 corners=((3, 2), (19, 5)))
    _CACHE["tilted"] = _frozen(case)
    return case


def all_cases():
    return dict(sheet=sheet_case(), lattice=lattice_case(), main=main_case(), mixed=mixed_case(), wide=wide_case(), pile=pile_case(),
                sphere=sphere_case(), tilted=tilted_case())
