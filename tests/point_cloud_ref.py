"""Yardsticks of coponerf_amd/point_cloud.py (csrc/point_cloud.hip) and the inputs of its tests: float64 numpy restatements of the
three rules of include/coponerf_hip.h (round 15), in the kernels' own operation order (sums left to right, one IEEE rounding per
operation), and the analytic scenes.  tests/test_point_cloud_ref.py holds them to independent forms on the CPU.

Bounds (U = 2^-24, E = 2^-53), from operation counts, none from a run:
  points        |kernel - float64| <= ulp32(|ref|) / 2 + 8 E M.  M = |R_r0 p_0| + |R_r1 p_1| + |R_r2 p_2| + |t_r| is the sum of the
                absolute terms of the component; p_0 = d ((u - cx) / fx) carries three roundings and its product with R_r0 a
                fourth, the three additions one each: (4 + 3) E M to first order, 8 E M with room for the second.
  depth_fused   |kernel - float64| <= ulp32(|ref|) / 2 + FUSED_OPS E M'.  The round trip of one view b is, along its longest path,
                7 (point) + 11 (into b) + 4 (project) + 2 (window) + 9 (bilinear) + 7 (ray and point) + 11 (into a) operations,
                FUSED_OPS = 51 + K for the sum over the views and the division; M' is the largest sum of absolute terms any stage
                of the trip forms, the pixel coordinates (the largest numbers in it) included.  The restatement runs the
                kernel's own operation sequence, so the two float64 values agree far inside E-sized terms; the part of the
                bound that bites is the one fp32 rounding of the store.
  votes         equal wherever no decision of the pixel lies within BAND = 1e-9 (relative) of its threshold; the tests count
                the pixels in the band and hold their share to BAND_SHARE = 1e-3.
"""
import numpy as np

from tests import novel_views_ref as nr

U = 2.0 ** -24
E = 2.0 ** -53
BAND = 1e-9
BAND_SHARE = 1e-3
POINT_OPS = 8
PX_TOL, REL_TOL = 1.0, 0.01


def fused_ops(K):
    return 51 + K


def valid(d):
    """The validity rule: finite and strictly inside depth_ray's clamp range."""
    d = np.asarray(d)
    with np.errstate(invalid="ignore"):
        return np.isfinite(d) & (d > 0) & (d < 10)


def window_of(S, window):
    return (0, 0, S, S) if window is None else tuple(int(v) for v in window)


def pixel_grid(S, window):
    """(u, v) float64 of the h * w pixels of the window, row-major."""
    y0, x0, h, w = window_of(S, window)
    v, u = np.divmod(np.arange(h * w), w)
    return (x0 + u).astype(np.float64), (y0 + v).astype(np.float64)


def cam_of(K44):
    K44 = np.asarray(K44, dtype=np.float32).astype(np.float64)
    return K44[0, 0], K44[1, 1], K44[0, 2], K44[1, 2]


def on_ray(cam, u, v, d):
    fx, fy, cx, cy = cam
    return [d * ((u - cx) / fx), d * ((v - cy) / fy), d]


def to_reference(P, p):
    """X = R p + t, left to right -> (X, the sum of the absolute terms of each component)."""
    X = [((P[r, 0] * p[0] + P[r, 1] * p[1]) + P[r, 2] * p[2]) + P[r, 3] for r in range(3)]
    M = [np.abs(P[r, 0] * p[0]) + np.abs(P[r, 1] * p[1]) + np.abs(P[r, 2] * p[2]) + np.abs(P[r, 3]) for r in range(3)]
    return X, M


def to_camera(P, X):
    """Y = R^T X + (-(R^T t)) -> (Y, the sum of the absolute terms of each component)."""
    Y, M = [], []
    for r in range(3):
        ti = -((P[0, r] * P[0, 3] + P[1, r] * P[1, 3]) + P[2, r] * P[2, 3])
        Y.append(((P[0, r] * X[0] + P[1, r] * X[1]) + P[2, r] * X[2]) + ti)
        M.append(np.abs(P[0, r] * X[0]) + np.abs(P[1, r] * X[1]) + np.abs(P[2, r] * X[2]) + np.abs(P[0, r] * P[0, 3]) +
                 np.abs(P[1, r] * P[1, 3]) + np.abs(P[2, r] * P[2, 3]))
    return Y, M


def project(cam, Y):
    fx, fy, cx, cy = cam
    return (fx * Y[0]) / Y[2] + cx, (fy * Y[1]) / Y[2] + cy


def half_ulp32(x):
    return 0.5 * np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def depth_points(depth, poses, intrinsics, S, window=None):
    """depth (K, B, h w) fp32, poses (K, B, 4, 4) fp32, intrinsics (B, 4, 4) fp32 -> (xyz (K, B, h w, 3) float64 with NaN where the
    depth is not valid, bound (K, B, h w, 3): what an fp32 store of a float64 evaluation may differ by)."""
    depth = np.asarray(depth, dtype=np.float32)
    K, B, R = depth.shape
    u, v = pixel_grid(S, window)
    xyz = np.full((K, B, R, 3), np.nan)
    bound = np.zeros((K, B, R, 3))
    P64 = np.asarray(poses, dtype=np.float32).astype(np.float64)
    for k in range(K):
        for b in range(B):
            ok = valid(depth[k, b])
            d = np.where(ok, depth[k, b], 1.0).astype(np.float64)
            X, M = to_reference(P64[k, b], on_ray(cam_of(intrinsics[b]), u, v, d))
            for r in range(3):
                xyz[k, b, :, r] = np.where(ok, X[r], np.nan)
                bound[k, b, :, r] = half_ulp32(X[r]) + POINT_OPS * E * M[r]
    return xyz, bound


def depth_votes(depth, poses, intrinsics, S, px_tol=PX_TOL, rel_tol=REL_TOL, window=None):
    """The vote rule.  Returns a dict:
      votes (K, B, R) uint8, fused (K, B, R) float64 (NaN where invalid), fused_bound (K, B, R),
      decided (K, K, B, R) bool: d_a valid and b != a;  consistent (K, K, B, R) bool;
      behind (K, K, B, R) bool: Y_z <= 0 in view b;  near (K, K, B, R) bool: a threshold decision inside the band."""
    depth = np.asarray(depth, dtype=np.float32)
    K, B, R = depth.shape
    y0, x0, h, w = window_of(S, window)
    u, v = pixel_grid(S, window)
    P64 = np.asarray(poses, dtype=np.float32).astype(np.float64)
    votes = np.zeros((K, B, R), dtype=np.uint8)
    fused = np.full((K, B, R), np.nan)
    fbound = np.zeros((K, B, R))
    decided = np.zeros((K, K, B, R), dtype=bool)
    consistent, behind, near = decided.copy(), decided.copy(), decided.copy()
    for a in range(K):
        for b in range(B):
            cam = cam_of(intrinsics[b])
            ok = valid(depth[a, b])
            da = np.where(ok, depth[a, b], 1.0).astype(np.float64)
            X, M = to_reference(P64[a, b], on_ray(cam, u, v, da))
            mag = np.maximum.reduce(M + [np.abs(u) + np.abs(cam[2]), np.abs(v) + np.abs(cam[3])])
            total, n = da.copy(), np.zeros(R, dtype=np.int64)
            for kb in range(K):
                if kb == a:
                    continue
                decided[a, kb, b] = ok
                with np.errstate(all="ignore"):
                    Y, My = to_camera(P64[kb, b], X)
                    front = ok & (Y[2] > 0.0)
                    behind[a, kb, b] = ok & ~(Y[2] > 0.0)
                    qx, qy = project(cam, Y)
                    wx, wy = qx - float(x0), qy - float(y0)
                    inside = front & (wx >= 0.0) & (wx < float(w - 1)) & (wy >= 0.0) & (wy < float(h - 1))
                    ix = np.where(inside, wx, 0.0).astype(np.int64)
                    iy = np.where(inside, wy, 0.0).astype(np.int64)
                    D = depth[kb, b].reshape(h, w)
                    ix1, iy1 = np.minimum(ix + 1, w - 1), np.minimum(iy + 1, h - 1)        # only read where `inside`
                    d00, d01, d10, d11 = D[iy, ix], D[iy, ix1], D[iy1, ix], D[iy1, ix1]
                    taps = inside & valid(d00) & valid(d01) & valid(d10) & valid(d11)
                    ax, ay = wx - ix, wy - iy
                    f = lambda t: np.where(taps, t, 1.0).astype(np.float64)
                    db = (1.0 - ay) * ((1.0 - ax) * f(d00) + ax * f(d01)) + ay * ((1.0 - ax) * f(d10) + ax * f(d11))
                    X2, M2 = to_reference(P64[kb, b], on_ray(cam, qx, qy, db))
                    Y2, M3 = to_camera(P64[a, b], X2)
                    back = taps & (Y2[2] > 0.0)
                    bx, by = project(cam, Y2)
                    ex, ey = bx - u, by - v
                    dist = np.sqrt(ex * ex + ey * ey)
                    dz = np.abs(Y2[2] - da)
                    yes = back & (dist <= px_tol) & (dz <= rel_tol * da)
                    near[a, kb, b] = back & ((np.abs(dist - px_tol) <= BAND * px_tol) |
                                             (np.abs(dz - rel_tol * da) <= BAND * rel_tol * da))
                    stage = np.maximum.reduce(My + M2 + M3 + [np.abs(qx) + np.abs(cam[2]), np.abs(qy) + np.abs(cam[3]),
                                                              np.abs(bx) + np.abs(cam[2]), np.abs(by) + np.abs(cam[3])])
                    mag = np.where(back, np.maximum(mag, np.where(back, stage, 0.0)), mag)
                consistent[a, kb, b] = yes
                total = np.where(yes, total + np.where(yes, Y2[2], 0.0), total)
                n += yes
            val = total / (1 + n).astype(np.float64)
            votes[a, b] = np.where(ok, n, 0)
            fused[a, b] = np.where(ok, val, np.nan)
            fbound[a, b] = half_ulp32(val) + fused_ops(K) * E * np.maximum(mag, np.abs(total))
    return {"votes": votes, "fused": fused, "fused_bound": fbound, "decided": decided, "consistent": consistent, "behind": behind,
            "near": near}


def compact(keep, xyz, rgb):
    """The compaction rule: per pair b the selected points in (view, row, column) order -> (list of (n_b, 3) float32, list of
    (n_b, 3) uint8 by cpn_pack_frames' byte rule, counts (B) int32).  Written with an explicit running output row, NOT boolean
    indexing: tests/test_point_cloud_ref.py holds it to that."""
    keep, xyz, rgb = np.asarray(keep), np.asarray(xyz, dtype=np.float32), np.asarray(rgb, dtype=np.float32)
    K, B, R = keep.shape
    out_xyz, out_rgb, counts = [], [], np.zeros(B, dtype=np.int32)
    for b in range(B):
        flags = (keep[:, b].reshape(K * R) != 0).astype(np.int64)
        row = np.cumsum(flags) - flags                                   # output row of every selected element
        n = int(flags.sum())
        ox, oc = np.empty((n, 3), dtype=np.float32), np.empty((n, 3), dtype=np.uint8)
        src = np.flatnonzero(flags)
        ox[row[src]] = xyz[:, b].reshape(K * R, 3)[src]
        oc[row[src]] = nr.to_byte((rgb[:, b].reshape(K * R, 3)[src] + np.float32(1)) * np.float32(127.5))
        out_xyz.append(ox)
        out_rgb.append(oc)
        counts[b] = n
    return out_xyz, out_rgb, counts


# ------------------------------------------------------------------------------------------------------------------ scenes
PLANE_N, PLANE_C = np.array([-0.3, -0.2, 1.0]), 4.0                  # the tilted plane z = 4 + 0.3 x + 0.2 y
BALL_C, BALL_R = np.array([0.1, 0.0, 2.6]), 0.5                      # the sphere in front of it


def rigid(deg_xyz, t):
    """(4, 4) float32: rotations about x, y and z (degrees, applied in that order) and a translation."""
    R = np.eye(3)
    for axis, deg in zip(np.eye(3), deg_xyz):
        R = nr.rotation_about(axis, np.radians(deg)) @ R
    P = np.eye(4)
    P[:3, :3], P[:3, 3] = R, t
    return P.astype(np.float32)


def cast(pose, cam, u, v):
    """Float64 ray casting of the scene from the camera `pose` (fp32 entries, taken as they are): the z-depth of the nearest
    hit of every pixel's ray and the surface it lies on (0 the plane, 1 the sphere)."""
    P = np.asarray(pose, dtype=np.float32).astype(np.float64)
    fx, fy, cx, cy = cam
    ray = np.stack(((u - cx) / fx, (v - cy) / fy, np.ones_like(u)), axis=-1)
    dirs, org = ray @ P[:3, :3].T, P[:3, 3]
    lam_plane = (PLANE_C - PLANE_N @ org) / (dirs @ PLANE_N)
    oc = org - BALL_C
    qa, qb, qc = (dirs * dirs).sum(-1), 2.0 * (dirs @ oc), oc @ oc - BALL_R ** 2
    disc = qb * qb - 4.0 * qa * qc
    with np.errstate(invalid="ignore"):
        lam_ball = np.where(disc > 0, (-qb - np.sqrt(np.abs(disc))) / (2.0 * qa), np.inf)
    ball = lam_ball < lam_plane
    return np.where(ball, lam_ball, lam_plane), ball.astype(np.int64)


MAIN = dict(S=72, window=(5, 9, 37, 53))
_INTR = ((60.0, 66.0, 37.3, 34.1), (75.0, 70.0, 33.5, 38.2))        # fx != fy, the principal point off centre
_MOVES = (((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)), ((-2.0, 4.0, 0.0), (0.30, 0.05, -0.10)), ((0.0, -3.0, 3.0), (-0.25, 0.20, 0.30)))
_CACHE = {}


def scene(K=3, B=2, S=72, window=(5, 9, 37, 53), planted=False):
    """dict of depth (K, B, h w) fp32 (ray-cast in float64, rounded once), true (the float64 depths), surface (K, B, h w),
    poses (K, B, 4, 4) fp32, intrinsics (B, 4, 4) fp32, S, window.  Pair 1's cameras move 0.8 times as far as pair 0's.
    planted=True writes the main case's faults into the depth (see plant)."""
    key = (K, B, S, window, planted)
    if key in _CACHE:
        return _CACHE[key]
    y0, x0, h, w = window_of(S, window)
    u, v = pixel_grid(S, window)
    intr = np.zeros((B, 4, 4), dtype=np.float32)
    poses = np.zeros((K, B, 4, 4), dtype=np.float32)
    true = np.zeros((K, B, h * w))
    surface = np.zeros((K, B, h * w), dtype=np.int64)
    for b in range(B):
        fx, fy, cx, cy = (c * S / 72.0 for c in _INTR[b])
        intr[b] = np.array([[fx, 0, cx, 0], [0, fy, cy, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float32)
        for k in range(K):
            deg, t = _MOVES[k]
            poses[k, b] = rigid(deg, np.array(t) * (1.0 - 0.2 * b))
            true[k, b], surface[k, b] = cast(poses[k, b], cam_of(intr[b]), u, v)
    depth = true.astype(np.float32)
    if planted:
        plant(depth.reshape(K, B, h, w))
    out = dict(depth=depth, true=true, surface=surface, poses=poses, intrinsics=intr, S=S, window=window, h=h, w=w)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    _CACHE[key] = out
    return out


# view, rows, columns of the patch scaled by 1.2: on the plane, clear of the sphere's silhouette (rows 17 and below) - across a
# depth edge the bilinear lookup blends the two surfaces and CAN land on a wrong depth, which is the rule, not a fault of it
PATCH = (1, slice(6, 14), slice(4, 44))
NEAR_ROW = (0, 35, slice(5, 15))                                     # depths of 0.05 .. 0.2: behind camera 2, which stands 0.3 ahead


def plant(d):
    """The main case's faults, in place in d (K, B, h, w): a patch of view 1 scaled by 1.2 (it must lose its votes), a row of NaN
    and one of near depths in view 0, a row of 0 in view 1, a row of exactly 10 and one +inf in view 2."""
    K = d.shape[0]                                                   # a case of fewer views keeps the faults of the views it has
    d[0, :, 2, :] = np.nan
    d[NEAR_ROW[0], :, NEAR_ROW[1], NEAR_ROW[2]] = np.linspace(0.05, 0.2, 10, dtype=np.float32)
    if K > 1:
        d[PATCH[0], :, PATCH[1], PATCH[2]] *= np.float32(1.2)
        d[1, :, 33, :] = 0.0
    if K > 2:
        d[2, :, 5, :] = 10.0
        d[2, :, 20, 40] = np.inf


def main_case():
    return scene(planted=True, **MAIN)


def clean_case():
    return scene(planted=False, **MAIN)


def further_cases():
    """name -> case: one view (every vote is 0), two views, and the whole grid of a 24 x 24 image."""
    return {"K1": scene(K=1, planted=True, **MAIN), "K2": scene(K=2, planted=True, **MAIN),
            "whole": scene(K=3, B=2, S=24, window=None)}


def all_cases():
    return dict(main=main_case(), **further_cases())


def votes_of(case):
    """depth_votes of a case at the default thresholds, computed once."""
    key = ("votes", id(case))
    if key not in _CACHE:
        _CACHE[key] = depth_votes(case["depth"], case["poses"], case["intrinsics"], case["S"], window=case["window"])
    return _CACHE[key]


def colours(shape, seed=7):
    """fp32 colours in [-1.1, 1.1] with a few NaN: the rgb input of the compaction tests."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1.1, 1.1, size=shape).astype(np.float32)
    c.reshape(-1)[::97] = np.nan
    return c
