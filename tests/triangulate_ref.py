"""Yardstick of coponerf_amd.triangulate (csrc/triangulate.hip, round 26 of include/coponerf_hip.h): a numpy float64 restatement of
cpn_triangulate_matches and cpn_depth_scale, operation by operation, for ONE pair, and of the keep rule of triangulate.cloud.
tests/test_triangulate_ref.py pins it on the CPU against forms it shares no code with (the epipolar constraint, Hartley and Sturm's
degree-6 polynomial, a DLT by SVD, the scene's true points, np.sort); tests/test_gpu_triangulate.py compares the kernels with it.

The residual pieces are tests/matches_ref.py's essential / sampson (round 16), whose bits the kernels of the earlier rounds already
reproduce; the two depth numerators are tests/ransac_ref.py's depths (round 20); the rank of depth_scale comes from
np.sort(kind="stable") under tests/pose_eval_ref.py's rank rule, and pose_eval_ref.radix_select restates the descent beside it; the
compaction of the cloud is tests/point_cloud_ref.py's.  numpy float64 arithmetic is IEEE, one rounding per operation, which is what
-ffp-contract=off gives the kernel: xyz, z0, z1, the error, the flags, the scale and the spread are compared in their bits, once the
fixtures have been shown to keep every decision at least MARGIN from its threshold (margins); the parallax takes an atan2 and is
held to 1 fp32 ulp.
"""
import functools

import numpy as np

from tests import lo_msac_ref as lm
from tests import matches_ref as mr
from tests import point_cloud_ref as pr
from tests import pose_eval_ref as pe
from tests import ransac_ref as rr

MARGIN = 1e-9
PASSES = 3
DEG = 57.29577951308232
INPUT, CORRECTION, PARALLAX, BEHIND0, BEHIND1 = 1, 2, 4, 8, 16
DEFECTS = ("two passes", "stale n", "z1 operand")                   # of triangulate; depth_scale has "upper median", "floor pixel"


def _cross(u, v):
    return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])


def _dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def bilinear(img, x, y):
    """The header's bilinear sample of img (S, S, 3) at the points (x, y) (n) float64 -> (n, 3) float64."""
    S = img.shape[0]
    img = np.asarray(img, dtype=np.float32).astype(np.float64)
    u, v = np.minimum(np.maximum(x, 0.0), S - 1.0), np.minimum(np.maximum(y, 0.0), S - 1.0)
    ix, iy = np.minimum(np.floor(u).astype(np.int64), max(S - 2, 0)), np.minimum(np.floor(v).astype(np.int64), max(S - 2, 0))
    jx, jy = np.minimum(ix + 1, S - 1), np.minimum(iy + 1, S - 1)
    lx, ly = (u - ix)[:, None], (v - iy)[:, None]
    return (1.0 - ly) * ((1.0 - lx) * img[iy, ix] + lx * img[iy, jx]) + ly * ((1.0 - lx) * img[jy, ix] + lx * img[jy, jx])


def correct(xy, intrinsics, pose, passes=PASSES, defect=None):
    """The correction of cpn_triangulate_matches on the rows xy (n, 4) float64 (all finite) under pose (4, 4) float64 -> dict:
    `D` (n, 4) the shifts (D_0, D_1, D'_0, D'_1) of the last pass, `xh` (n, 4) the corrected match, `failed` (n) bool, `trace`:
    per pass the dict of A, Bq, disc, den, lam and the shifts - what the CPU tests read -, `F` (3, 3) = K0^-T E K1^-1 formed as
    the kernel forms its pieces, `c` (n).  defect="stale n": n and n' are refreshed from themselves, not from n0 and n0'."""
    k0, k1 = mr.cam_of(intrinsics[0]), mr.cam_of(intrinsics[1])
    R, t = pose[:3, :3], pose[:3, 3]
    tl = np.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2])
    Em = mr.essential(R, t / tl)
    x0, y0, x1, y1 = (xy[:, i] for i in range(4))
    s = mr.sampson(Em, k0, k1, x0, y0, x1, y1)
    c = s["n"]
    f0, f1 = (k0[0], k0[1]), (k1[0], k1[1])
    Ft = [[(Em[i, j] / f0[i]) / f1[j] for j in range(2)] for i in range(2)]
    p, q = (s["g"][0], s["g"][1]), (s["g"][2], s["g"][3])               # n0 and n0'
    n, m = p, q
    failed, trace = np.zeros(len(xy), dtype=bool), []
    D = G = (np.zeros(len(xy)), np.zeros(len(xy)))
    for _ in range(passes):
        A = n[0] * (Ft[0][0] * m[0] + Ft[0][1] * m[1]) + n[1] * (Ft[1][0] * m[0] + Ft[1][1] * m[1])
        Bq = 0.5 * ((n[0] * p[0] + n[1] * p[1]) + (m[0] * q[0] + m[1] * q[1]))
        disc = Bq * Bq - A * c
        d = np.sqrt(disc)
        den = Bq + d
        lam = c / den
        failed = failed | ~(disc >= 0.0) | ~(den != 0.0)
        D, G = (lam * n[0], lam * n[1]), (lam * m[0], lam * m[1])
        trace.append({"A": A, "Bq": Bq, "disc": disc, "den": den, "lam": lam, "D": np.stack(D + G, 1)})
        base_n, base_m = (n, m) if defect == "stale n" else (p, q)
        n = (base_n[0] - (Ft[0][0] * G[0] + Ft[0][1] * G[1]), base_n[1] - (Ft[1][0] * G[0] + Ft[1][1] * G[1]))
        m = (base_m[0] - (Ft[0][0] * D[0] + Ft[1][0] * D[1]), base_m[1] - (Ft[0][1] * D[0] + Ft[1][1] * D[1]))
    F = np.array([[Em[i, j] / ((f0 + (1.0,))[i] * (f1 + (1.0,))[j]) for j in range(3)] for i in range(3)])
    C0, C1 = np.array([[1, 0, -k0[2]], [0, 1, -k0[3]], [0, 0, 1.0]]), np.array([[1, 0, -k1[2]], [0, 1, -k1[3]], [0, 0, 1.0]])
    F = C0.T @ F @ C1                                                   # for the CPU tests alone: x^T F x' in pixels
    shifts = np.stack(D + G, 1)
    return {"D": shifts, "xh": xy - shifts, "failed": failed, "trace": trace, "F": F, "c": c}


def rows64(m, K, P, passes=PASSES, defect=None):
    """Everything cpn_triangulate_matches computes for the finite rows m (n, 4) float64 under cameras K (2, 4, 4) and pose P
    (4, 4), float64 -> (xyz (n, 3), geom (n, 4), flag (n) uint8, xh (n, 4), disc_rel (n): the smallest disc / Bq^2 of the passes).
    The CPU tests call it with float64 coordinates; triangulate() with the fp32 ones."""
    k0, k1 = mr.cam_of(K[0]), mr.cam_of(K[1])
    R, t = P[:3, :3], P[:3, 3]
    co = correct(m, K, P, passes - 1 if defect == "two passes" else passes, defect)
    h = co["xh"]
    ah = ((h[:, 0] - k0[2]) / k0[0], (h[:, 1] - k0[3]) / k0[1], np.ones(len(m)))
    bh0, bh1 = (h[:, 2] - k1[2]) / k1[0], (h[:, 3] - k1[3]) / k1[1]
    cr = [(R[j, 0] * bh0 + R[j, 1] * bh1) + R[j, 2] for j in range(3)]
    w = _cross(ah, cr)
    ww = _dot(w, w)
    z0n, z1n = rr.depths(R, t, ah[0], ah[1], bh0, bh1)                  # (t x cr) . w and (t x ah) . w
    if defect == "z1 operand":
        z1n = z0n
    z0, z1 = z0n / ww, z1n / ww
    D = co["D"]
    err = np.sqrt(((D[:, 0] * D[:, 0] + D[:, 1] * D[:, 1]) + D[:, 2] * D[:, 2]) + D[:, 3] * D[:, 3])
    par = np.arctan2(np.sqrt(ww), _dot(ah, cr)) * DEG
    flag = (np.where(co["failed"], CORRECTION, 0) | np.where(~(ww > 0.0), PARALLAX, 0) | np.where(~(z0 > 0.0), BEHIND0, 0) |
            np.where(~(z1 > 0.0), BEHIND1, 0)).astype(np.uint8)
    disc_rel = np.min([tr["disc"] / (tr["Bq"] * tr["Bq"]) for tr in co["trace"]], axis=0) if co["trace"] else np.ones(len(m))
    return np.stack((z0 * ah[0], z0 * ah[1], z0), 1), np.stack((z0, z1, err, par), 1), flag, h, disc_rel


def triangulate(xy, count, intrinsics, pose, images=None, passes=PASSES, defect=None):
    """The rule of cpn_triangulate_matches for ONE pair: xy (N, 4) fp32, count, intrinsics (2, 4, 4) fp32, pose (4, 4) fp32,
    images None or (2, S, S, 3) fp32 -> dict of `xyz` (N, 3) fp32, `geom` (N, 4) fp32, `flag` (N) uint8, `rgb` (N, 3) fp32 with
    images, and the float64 values before the store: `xyz64`, `geom64`, `xh` (N, 4), `disc_rel` (N) (NaN where the row was not
    computed).  defect: "two passes" (one pass short), "stale n" (correct's), "z1 operand" (z1 from t x cr instead of t x ah)."""
    xy32 = np.asarray(xy, dtype=np.float32)
    N = len(xy32)
    n = min(max(int(count), 0), N)
    P = np.asarray(pose, dtype=np.float32).astype(np.float64)
    K = np.asarray(intrinsics, dtype=np.float32).astype(np.float64)
    xyz64, geom64, xh, disc_rel = np.full((N, 3), np.nan), np.full((N, 4), np.nan), np.full((N, 4), np.nan), np.full(N, np.nan)
    flag = np.full(N, 255, dtype=np.uint8)
    flag[:n] = INPUT
    pair_ok = np.isfinite(P[:3]).all() and P[:3, 3].any() and np.isfinite(mr.cam_of(K[0]) + mr.cam_of(K[1])).all()
    rows = np.flatnonzero(np.isfinite(xy32[:n]).all(axis=1)) if pair_ok else np.zeros(0, dtype=np.int64)
    m = xy32[rows].astype(np.float64)
    with np.errstate(all="ignore"):
        if len(rows):
            xyz64[rows], geom64[rows], flag[rows], xh[rows], disc_rel[rows] = rows64(m, K, P, passes, defect)
        out = {"xyz": xyz64.astype(np.float32), "geom": geom64.astype(np.float32), "flag": flag, "xyz64": xyz64, "geom64": geom64, "xh": xh,
               "disc_rel": disc_rel}
        if images is not None:
            rgb = np.full((N, 3), np.nan)
            if len(rows):
                rgb[rows] = 0.5 * (bilinear(images[0], m[:, 0], m[:, 1]) + bilinear(images[1], m[:, 2], m[:, 3]))
            out["rgb"] = rgb.astype(np.float32)
    return out


def keep_mask(geom, flag, max_reproj_px=1.0, min_parallax_deg=1.0, inlier=None):
    """The keep rule of triangulate.cloud on fp32 geom (N, 4) and flag (N): flag 0, error <= max_reproj_px, parallax >=
    min_parallax_deg (the fp32 values against the fp32 thresholds, as torch compares them), and inlier != 0 where given."""
    geom = np.asarray(geom, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        keep = (np.asarray(flag) == 0) & (geom[:, 2] <= np.float32(max_reproj_px)) & (geom[:, 3] >= np.float32(min_parallax_deg))
    return keep if inlier is None else keep & (np.asarray(inlier) != 0)


def cloud(tri, max_reproj_px=1.0, min_parallax_deg=1.0, inlier=None):
    """triangulate.cloud of ONE pair's triangulate() dict -> (xyz (k, 3) fp32, rgb (k, 3) uint8): the kept rows in their order,
    by tests/point_cloud_ref.py's compaction; grey (0) where the dict has no colours."""
    keep = keep_mask(tri["geom"], tri["flag"], max_reproj_px, min_parallax_deg, inlier)
    rgb = tri["rgb"] if "rgb" in tri else np.zeros_like(tri["xyz"])
    xyz, col, _ = pr.compact(keep[None, None].astype(np.uint8), tri["xyz"][None, None], rgb[None, None])
    return xyz[0], col[0]


def ratios(geom, flag, xy, count, depth, S, max_reproj_px=1.0, min_parallax_deg=1.0, defect=None):
    """(q (n) float64, used (n) bool) of cpn_depth_scale's rows below the count.  defect="floor pixel": the depth is read at
    (floor(x0), floor(y0))."""
    geom, xy = np.asarray(geom, dtype=np.float32), np.asarray(xy, dtype=np.float32)
    n = min(max(int(count), 0), len(xy))
    g, rows, f = geom[:n].astype(np.float64), xy[:n].astype(np.float64), np.asarray(flag)[:n]
    depth = np.asarray(depth, dtype=np.float32).reshape(S, S)
    half = 0.0 if defect == "floor pixel" else 0.5
    with np.errstate(all="ignore"):
        u, v = np.floor(rows[:, 0] + half), np.floor(rows[:, 1] + half)
        inside = (u >= 0.0) & (u <= S - 1.0) & (v >= 0.0) & (v <= S - 1.0)
        d = depth[np.where(inside, v, 0).astype(np.int64), np.where(inside, u, 0).astype(np.int64)]
        valid = (d > np.float32(0)) & (d < np.float32(10))
        q = d.astype(np.float64) / g[:, 0]
        used = (f == 0) & (g[:, 2] <= max_reproj_px) & (g[:, 3] >= min_parallax_deg) & inside & valid & np.isfinite(q) & (q > 0.0)
    return q, used


def depth_scale(geom, flag, xy, count, depth, S, rel_pose=None, max_reproj_px=1.0, min_parallax_deg=1.0, min_rows=8, defect=None):
    """The rule of cpn_depth_scale for ONE pair -> (scale float64, stats (4) float64).  defect: "upper median" (rank n_u / 2
    rounded down of both medians), "floor pixel" (ratios')."""
    q, used = ratios(geom, flag, xy, count, depth, S, max_reproj_px, min_parallax_deg, defect)
    n_u = int(used.sum())
    if n_u < min_rows:
        return np.nan, np.array([float(n_u), np.nan, np.nan, 1.0])
    rank = n_u >> 1 if defect == "upper median" else (n_u - 1) >> 1
    scale = np.sort(q[used], kind="stable")[rank]
    spread = np.sort(np.abs(q[used] / scale - 1.0), kind="stable")[rank]
    length = np.nan
    if rel_pose is not None:
        t = np.asarray(rel_pose, dtype=np.float32).astype(np.float64)[:3, 3]
        length = np.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2])
    return scale, np.array([float(n_u), spread, length / scale, 0.0])


def margins(tri, max_reproj_px=1.0, min_parallax_deg=1.0):
    """The smallest distance of a computed row of triangulate()'s dict from a decision: the error from max_reproj_px, the
    parallax from min_parallax_deg, z0 and z1 from 0, and disc / Bq^2 of every pass from 0 (rows with a value that is exactly 0
    or not a number are decided by construction, not by rounding, and are left out)."""
    g = tri["geom64"]
    on = np.isfinite(g).all(axis=1)
    z = g[on][:, :2]
    z = z[z != 0.0]
    disc = tri["disc_rel"][np.isfinite(tri["disc_rel"]) & (tri["disc_rel"] != 0.0)]
    return float(min(np.abs(g[on, 2] - max_reproj_px).min(), np.abs(g[on, 3] - min_parallax_deg).min(), np.abs(z).min(), np.abs(disc).min()))


def unit(pose):
    """[R | t / |t|] of a (4, 4) pose, fp32."""
    P = np.asarray(pose, dtype=np.float64).copy()
    P[:3, 3] /= np.linalg.norm(P[:3, 3])
    return P.astype(np.float32)


# -------------------------------------------------------------------------------------------------------------- the fixtures
S_GPU = 256


@functools.lru_cache(maxsize=None)
def scene_case():
    """lo_msac_ref.gpu_case() - B = 2, N = 768, counts 257 and 511: more rows than a workgroup, no multiple of 256 - with NaN at
    and beyond the counts, pair 0 under the scene's true pose and pair 1 under the same with |t| = 1, and two random photos.
    -> (xy, counts, intrinsics, poses (2, 4, 4) fp32, images (2, 2, S, S, 3) fp32 with S = 32: the matches beyond it clamp)."""
    xy, counts, K, _ = lm.gpu_case()
    xy = xy.copy()
    for b, c in enumerate(counts):
        xy[b, c:] = np.nan
    truth = rr.true_pose(lm.scene("curved"))
    images = np.random.default_rng(26).uniform(-1.0, 1.0, (2, 2, 32, 32, 3)).astype(np.float32)
    return xy, counts, K, np.stack((truth, unit(truth))), images


ROWS = ("exact", "epipole", "no parallax", "behind one", "behind both", "nan", "outlier")


@functools.lru_cache(maxsize=None)
def constructed_case():
    """B = 2, N = 300, counts 300 and 8, cameras f = 200, c = 128, R = 1 and t = (0, 0, 1) for pair 0, (0, 0, -1) for pair 1: E has
    the entries 0 and +-1, both epipoles are the principal point, and a pair of pixels on one line through it has c = 0 exactly.
    Rows 0 .. 6 of both pairs are ROWS: an exact match (a = (1/8, 1/4), b = (1/4, 1/2): z0 = 2, z1 = 1 under pair 0's pose), both
    epipoles, the same pixel twice (no parallax), a point behind one camera for each sign of t, a NaN, and an exact match moved
    176 px in view 1.  The other rows of pair 0 are exact matches of random points with 0.3 px of noise.
    -> (xy (2, 300, 4) fp32, counts, intrinsics (2, 2, 4, 4), poses (2, 4, 4))."""
    rng = np.random.default_rng(260)
    f, c, N = 200.0, 128.0, 300
    K = np.stack([np.stack((mr.pinhole(f, 256), mr.pinhole(f, 256)))] * 2)
    poses = np.stack((np.eye(4), np.eye(4))).astype(np.float32)
    poses[0, 2, 3], poses[1, 2, 3] = 1.0, -1.0
    xy = np.full((2, N, 4), np.nan, dtype=np.float32)
    px = lambda a: (c + f * a[0], c + f * a[1])
    for b in range(2):
        tz = float(poses[b, 2, 3])
        a = rng.uniform(-0.5, 0.5, (N, 2))
        z0 = rng.uniform(2.5, 6.0, N)
        z1 = z0 - tz                                                    # X0 = X1 + t
        pb = a * (z0 / z1)[:, None]
        rows = np.concatenate((c + f * a, c + f * pb + rng.normal(scale=0.3, size=(N, 2))), 1)
        xy[b] = rows.astype(np.float32)
        near, far = (0.125, 0.25), (0.25, 0.5)                          # z0 = 2, z1 = 1 for t_z = 1; z0 = 1, z1 = 2 for t_z = -1
        first, second = (near, far) if tz > 0 else (far, near)
        xy[b, 0] = px(first) + px(second)
        xy[b, 1] = (c, c, c, c)
        xy[b, 2] = px(near) + px(near)
        # X0_z = t_z / 2: in front of camera 0 and behind camera 1 for t_z = 1, the other way round for -1; then a point behind both
        for row, depth0 in ((3, 0.5 * tz), (4, -0.5 if tz > 0 else -1.5)):
            X0 = np.array([0.1, 0.05, depth0])
            X1 = X0 - np.array([0.0, 0.0, tz])
            xy[b, row] = px(X0[:2] / X0[2]) + px(X1[:2] / X1[2])
        xy[b, 5] = xy[b, 0]
        xy[b, 5, 2] = np.nan
        xy[b, 6] = xy[b, 0] + np.array([0.0, 0.0, 176.0, 0.0], dtype=np.float32)
    xy[1, 8:] = np.nan
    return xy, np.asarray((N, 8), dtype=np.int32), K, poses


@functools.lru_cache(maxsize=None)
def want_points(case):
    """triangulate() of every pair of scene_case ("scene", with colours) or constructed_case ("constructed").  Shared."""
    if case == "scene":
        xy, counts, K, poses, images = scene_case()
        return [triangulate(xy[b], counts[b], K[b], poses[b], images[b]) for b in range(2)]
    xy, counts, K, poses = constructed_case()
    return [triangulate(xy[b], counts[b], K[b], poses[b]) for b in range(2)]


def true_depth_map(scene_xy, depth, S):
    """(S S) fp32: 0 everywhere (not valid) but at the nearest pixel of every row's view-0 point, which holds the row's depth
    (a later row wins a shared pixel)."""
    out = np.zeros((S, S), dtype=np.float32)
    u, v = np.floor(scene_xy[:, 0].astype(np.float64) + 0.5).astype(np.int64), np.floor(scene_xy[:, 1].astype(np.float64) + 0.5).astype(np.int64)
    on = (u >= 0) & (u < S) & (v >= 0) & (v < S)
    out[v[on], u[on]] = depth[on]
    return out.reshape(-1)


def scene_depths(n=1000, seed=16, **_):
    """The true z-depth in view 0 of every row of matches_ref.refine_scene(n, seed, ..): its generator, drawn again (the test of
    the true points holds the two together)."""
    rng = np.random.default_rng(seed)
    rng.uniform(0.0, 256, size=(n, 2))
    return rng.uniform(1.0, 6.0, size=n)


@functools.lru_cache(maxsize=None)
def scale_case():
    """B = 6 pairs of N = 768 rows for cpn_depth_scale, S = 256: the noisy curved scene's first 768 rows triangulated under its
    true pose with |t| = 1 (the restatement's geom and flag), against true_depth_map of the scene's depths; counts 768, 0, 1, 7,
    8 and 768 with a pose of zero translation (every row flagged).  rel_pose: the truth.
    -> (geom (6, N, 4) fp32, flag (6, N) uint8, xy (6, N, 4) fp32, counts (6) int32, depth (6, S S) fp32, rel_pose (6, 4, 4))."""
    sc = lm.scene("curved")
    N, S = 768, S_GPU
    truth = rr.true_pose(sc)
    still = truth.copy()
    still[:3, 3] = 0.0
    depth = true_depth_map(sc["xy"][:N], scene_depths(**rr.NOISY)[:N].astype(np.float32), S)
    counts = (N, 0, 1, 7, 8, N)
    geoms, flags, xys = [], [], []
    for b, c in enumerate(counts):
        xy = sc["xy"][:N].copy()
        if b in (2, 3, 4):                                               # rows that the keep rule takes first: 1, 7 and 8 are n_u
            tri = triangulate(xy, N, sc["intrinsics"], unit(truth))
            q, used = ratios(tri["geom"], tri["flag"], xy, N, depth, S)
            xy = np.concatenate((xy[used], xy[~used]))
        xy[c:] = np.nan
        tri = triangulate(xy, c, sc["intrinsics"], still if b == 5 else unit(truth))
        geoms.append(tri["geom"])
        flags.append(tri["flag"])
        xys.append(xy)
    return (np.stack(geoms), np.stack(flags), np.stack(xys), np.asarray(counts, dtype=np.int32), np.stack([depth] * 6),
            np.stack([truth] * 6))


@functools.lru_cache(maxsize=None)
def want_scales():
    geom, flag, xy, counts, depth, rel = scale_case()
    return [depth_scale(geom[b], flag[b], xy[b], counts[b], depth[b], S_GPU, rel[b]) for b in range(len(xy))]
