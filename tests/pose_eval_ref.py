"""Yardstick of coponerf_amd.matches.pose_errors and residual_stats (csrc/pose_eval.hip, round 25 of include/coponerf_hip.h): a numpy
float64 restatement of both kernels, operation by operation, for ONE pair.  tests/test_pose_eval_ref.py pins it on the CPU;
tests/test_gpu_pose_eval.py compares the kernels with it.

The residual is tests/matches_ref.py's sampson / residual (round 16), whose bits the kernels of the earlier rounds already
reproduce; the rank of residual_stats comes from np.sort(kind="stable") and radix_select restates the kernel's descent beside it;
the sum of sigma[1] is matches_ref.block_sum, the order of a pass of cpn_refine_pose.  So usable, within, status, quant and both
sigmas are compared in their bits, once the fixtures have been shown to keep every |r| at least MARGIN from a threshold and from
the 2.5 sigma cut (threshold_margin); the angles of pose_errors take an atan2 and are held to 8 ulp.
"""
import functools

import numpy as np

from tests import lo_msac_ref as lm
from tests import matches_ref as mr
from tests import ransac_ref as rr

MARGIN = 1e-9
DEFECTS = ("upper median", "all rows", "strict")                    # of residual_stats; radix_select has "missing digit"


# ------------------------------------------------------------------------------------------------------------ pose errors
def _norm3(x, y, z):
    return np.sqrt((x * x + y * y) + z * z)


def pose_errors(poses, gt):
    """poses (P, 4, 4), gt (4, 4), fp32 values -> (P, 3) float64: cpn_pose_errors' three values in its operation order."""
    poses, G = np.asarray(poses, dtype=np.float32).astype(np.float64), np.asarray(gt, dtype=np.float32).astype(np.float64)
    out = np.full((len(poses), 3), np.nan)
    for p, A in enumerate(poses):
        if not (np.isfinite(A[:3]).all() and np.isfinite(G[:3]).all()):
            continue
        R, Rg, t, g = A[:3, :3], G[:3, :3], A[:3, 3], G[:3, 3]
        M = np.empty((3, 3))
        for i in range(3):
            for j in range(3):
                M[i, j] = (R[i, 0] * Rg[j, 0] + R[i, 1] * Rg[j, 1]) + R[i, 2] * Rg[j, 2]
        s = 0.5 * _norm3(M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1])
        c = (((M[0, 0] + M[1, 1]) + M[2, 2]) - 1.0) / 2.0
        out[p, 0] = np.arctan2(s, c)
        out[p, 1] = _norm3(t[0] - g[0], t[1] - g[1], t[2] - g[2])
        if t.any() and g.any():
            x = _norm3(t[1] * g[2] - t[2] * g[1], t[2] * g[0] - t[0] * g[2], t[0] * g[1] - t[1] * g[0])
            out[p, 2] = np.arctan2(x, (t[0] * g[0] + t[1] * g[1]) + t[2] * g[2])
    return out


def acos_rule64(poses, gt):
    """test.py's formula (evaluate.pose_metrics) in float64: acos of the cosines -> (P, 3)."""
    poses, G = np.asarray(poses, dtype=np.float64), np.asarray(gt, dtype=np.float64)
    out = np.empty((len(poses), 3))
    for p, A in enumerate(poses):
        M = A[:3, :3] @ G[:3, :3].T
        out[p, 0] = np.arccos(np.clip((np.trace(M) - 1.0) / 2.0, -1.0, 1.0))
        out[p, 1] = np.linalg.norm(A[:3, 3] - G[:3, 3])
        with np.errstate(all="ignore"):
            out[p, 2] = np.arccos(np.clip(A[:3, 3] / np.linalg.norm(A[:3, 3]) @ (G[:3, 3] / np.linalg.norm(G[:3, 3])), -1.0, 1.0))
    return out


def acos_rule32(poses, gt):
    """evaluate.pose_metrics' rotation angle as fp32 computes it: the product, the trace and the acos in fp32 -> (P,) fp32."""
    F = np.float32
    poses, G = np.asarray(poses, dtype=F), np.asarray(gt, dtype=F)
    out = np.empty(len(poses), dtype=F)
    for p, A in enumerate(poses):
        M = (A[:3, :3] @ G[:3, :3].T).astype(F)
        cos = F((F(F(M[0, 0] + M[1, 1]) + M[2, 2]) - F(1)) / F(2))
        out[p] = np.arccos(np.clip(cos, F(-1), F(1)))
    return out


def ulps(got, want):
    """|got - want| in units of want's last place (0 where both are NaN, inf where one is)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    both = np.isnan(got) & np.isnan(want)
    with np.errstate(all="ignore"):
        u = np.abs(got - want) / np.spacing(np.abs(want))
    return np.where(both, 0.0, np.where(np.isnan(u), np.inf, u))


# ------------------------------------------------------------------------------------------------------------ the selection
def keys_of(a):
    """The 64-bit patterns of |a|: non-negative doubles order as they do, and -0 and +0 are one key."""
    return np.abs(np.asarray(a, dtype=np.float64)).view(np.uint64)


def radix_select(values, k, defect=None):
    """The kernel's descent: the element of rank k of |values| (all usable), 8 bits a pass from the top; every pass counts the
    digits of the rows that carry the prefix found so far and takes the first digit whose rows reach beyond the rank.
    defect="missing digit": pass 5 is skipped, its digit stays 0."""
    keys = keys_of(values)
    prefix, rank = np.uint64(0), int(k)
    for p in range(8):
        if defect == "missing digit" and p == 5:
            continue
        shift = np.uint64(56 - 8 * p)
        head = keys >> (shift + np.uint64(8)) if p else np.zeros_like(keys)
        on = head == ((prefix >> (shift + np.uint64(8))) if p else np.uint64(0))
        hist = np.bincount(((keys[on] >> shift) & np.uint64(255)).astype(np.int64), minlength=256)
        below, d = 0, 0
        while d < 255 and not rank < below + hist[d]:
            below += int(hist[d])
            d += 1
        rank -= below
        prefix |= np.uint64(d) << shift
    return np.array([prefix], dtype=np.uint64).view(np.float64)[0]


def abs_residuals(xy, count, intrinsics, pose):
    """(|r| (n) float64, usable (n) bool) of the rows below the count under E = [t]x R of pose (4, 4) fp32, t as it comes."""
    xy = np.asarray(xy, dtype=np.float32)
    n = min(max(int(count), 0), len(xy))
    rows = xy[:n].astype(np.float64)
    P = np.asarray(pose, dtype=np.float32).astype(np.float64)
    k0, k1 = mr.cam_of(intrinsics[0]), mr.cam_of(intrinsics[1])
    with np.errstate(all="ignore"):
        s = mr.sampson(mr.essential(P[:3, :3], P[:3, 3]), k0, k1, rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3])
        r, ok = mr.residual(s)
    return np.abs(r), ok


def residual_stats(xy, count, intrinsics, poses, q=(0.5,), thr=(1.0,), defect=None):
    """The rule of cpn_residual_stats for one pair and poses (P, 4, 4) -> dict of usable (P) int32, quant (P, Q), within (P, T)
    int32, sigma (P, 2), status (P) int32, and cut (P), the 2.5 sigma[0] the second sigma cuts at.
    defect: "upper median" (rank ceil for q = 0.5 and the sigmas), "all rows" (the rank among all rows below the count, unusable
    ones sorted last), "strict" (< for <= at the thresholds and the cut)."""
    poses = np.asarray(poses, dtype=np.float32)
    P, Q, T = len(poses), len(q), len(thr)
    out = {"usable": np.zeros(P, dtype=np.int32), "quant": np.full((P, Q), np.nan), "within": np.zeros((P, T), dtype=np.int32),
           "sigma": np.full((P, 2), np.nan), "status": np.zeros(P, dtype=np.int32), "cut": np.full(P, np.nan)}
    le = (lambda a, b: a < b) if defect == "strict" else (lambda a, b: a <= b)
    for p, pose in enumerate(poses):
        A = pose.astype(np.float64)
        if not np.isfinite(A[:3]).all() or not A[:3, 3].any():
            out["status"][p] = 2
            continue
        a, ok = abs_residuals(xy, count, intrinsics, pose)
        n_u = int(ok.sum())
        if n_u == 0:
            out["status"][p] = 1
            continue
        ranked = np.sort(np.where(ok, a, np.inf), kind="stable")    # the usable ones first, ascending
        span = (len(a) if defect == "all rows" else n_u) - 1
        out["usable"][p] = n_u
        for j, qj in enumerate(q):
            k = int(np.ceil(qj * span)) if (defect == "upper median" and qj == 0.5) else int(np.floor(qj * span))
            out["quant"][p, j] = ranked[min(max(k, 0), span)]
        for t, px in enumerate(thr):
            out["within"][p, t] = int((ok & le(a, px)).sum())
        med = ranked[(span + 1) >> 1 if defect == "upper median" else span >> 1]
        if n_u > 5:
            s0 = (1.4826 * (1.0 + 5.0 / float(n_u - 5))) * med
            cut = 2.5 * s0
            inl = ok & le(a, cut)
            total = mr.block_sum(np.where(inl, a * a, 0.0)[:, None])[0]
            out["sigma"][p, 0], out["cut"][p] = s0, cut
            if int(inl.sum()) > 5:
                out["sigma"][p, 1] = np.sqrt(total / float(int(inl.sum()) - 5))
    return out


def threshold_margin(xy, count, intrinsics, poses, thr):
    """The smallest distance of a usable |r| from a threshold or from the 2.5 sigma[0] cut, over the poses (inf where there is
    none).  A level that is exactly 0 is left out: |r| <= 0 asks whether r IS 0, r = n / sqrt(D) is 0 iff n is, and no relative
    error of an evaluation turns a non-zero n into 0 or back (the shear rows' n is one exact difference of two fp32 values; the
    wide set's |r| go down to 1e-12 px on purpose)."""
    want = residual_stats(xy, count, intrinsics, poses, (0.5,), thr)
    least = np.inf
    for p, pose in enumerate(np.asarray(poses, dtype=np.float32)):
        if want["status"][p]:
            continue
        a, ok = abs_residuals(xy, count, intrinsics, pose)
        for level in tuple(thr) + ((want["cut"][p],) if np.isfinite(want["cut"][p]) else ()):
            if level != 0.0 and ok.any():
                least = min(least, float(np.abs(a[ok] - level).min()))
    return least


# ------------------------------------------------------------------------------------------------------------------ the AUC
def auc_brute(errors, t, cells=200000):
    """The area under the recall curve through (0, 0) and (e_i, i / n), flat from the last error below t, up to t and over t: a
    trapezoid rule on `cells` cells.  The curve is monotone with total variation <= 1, so the rule is off by at most t / cells in
    area: 1 / cells after the division."""
    e = np.sort(np.where(np.isnan(errors), np.inf, np.asarray(errors, dtype=np.float64)))
    n, m = len(e), int((e < t).sum())
    xs, ys = np.concatenate(([0.0], e[:m], [t])), np.concatenate(([0.0], np.arange(1, m + 1) / n, [m / n]))
    grid = np.linspace(0.0, t, cells + 1)
    v = np.interp(grid, xs, ys)
    return float(((v[1:] + v[:-1]) / 2.0).sum() * (t / cells) / t)


# -------------------------------------------------------------------------------------------------------------- the fixtures
Q_GPU, THR_GPU = (0.0, 0.5, 0.9, 1.0), (0.0, 1.0)
SHEAR_N = 600


def shear_pose():
    """R = 1, t = (-1, 0, 0): with shear_rows' cameras the residual of a row is (y0 - y1) / sqrt(2), whatever x0 and x1."""
    P = np.eye(4, dtype=np.float32)
    P[0, 3] = -1.0
    return P


def shear_rows(values, seed=0):
    """Rows (x0, 0, x1, v) for cameras with f = 1 and c = 0 (intrinsics the identity): under shear_pose n = -v and D = 2
    exactly, so r = -v / sqrt(2) for ANY fp32 v - residuals by construction."""
    rng = np.random.default_rng(seed)
    v = np.asarray(values, dtype=np.float32)
    xy = np.zeros((len(v), 4), dtype=np.float32)
    xy[:, 0], xy[:, 2], xy[:, 3] = rng.uniform(-1, 1, len(v)), rng.uniform(-1, 1, len(v)), v
    return xy


@functools.lru_cache(maxsize=None)
def residual_sets():
    """name -> SHEAR_N values of y1: all zero, tied (five values), wide (|v| = 10^u, u uniform in -12 .. 3, either sign: the
    exponent digits differ), random (gaussian)."""
    rng = np.random.default_rng(25)
    zero = np.zeros(SHEAR_N, dtype=np.float32)
    tied = rng.choice(np.array([0.25, 0.5, 0.75, 2.0, 7.0], dtype=np.float32), SHEAR_N)
    wide = (10.0 ** rng.uniform(-12.0, 3.0, SHEAR_N) * rng.choice((-1.0, 1.0), SHEAR_N)).astype(np.float32)
    return {"zero": zero, "tied": tied, "wide": wide, "random": rng.normal(scale=0.8, size=SHEAR_N).astype(np.float32)}


@functools.lru_cache(maxsize=None)
def shear_case():
    """The second batch of tests/test_gpu_pose_eval.py: B = 8 pairs of N = SHEAR_N rows - zero (count 300; every third row is
    (-0.5, -0, 0.5, 0), whose n is (-0 + -0) + -0: r = -0, the others' +0), tied, wide, random
    with a NaN row inside the count, and wide with counts 0, 1, 5 and 6; rows at and beyond the count are NaN.  P = 2 poses:
    shear_pose and the same without a translation (status 2).
    -> (xy (8, N, 4) fp32, counts (8) int32, intrinsics (8, 2, 4, 4) fp32, poses (8, 2, 4, 4) fp32).  Shared, never written to."""
    sets = residual_sets()
    names, counts = ("zero", "tied", "wide", "random", "wide", "wide", "wide", "wide"), (300, SHEAR_N, SHEAR_N, 400, 0, 1, 5, 6)
    xy = np.stack([shear_rows(sets[name], seed=b) for b, name in enumerate(names)])
    xy[0, ::3] = (-0.5, -0.0, 0.5, 0.0)
    xy[3, 123, 1] = np.nan
    for b, c in enumerate(counts):
        xy[b, c:] = np.nan
    still = np.eye(4, dtype=np.float32)
    K = np.broadcast_to(np.eye(4, dtype=np.float32), (8, 2, 4, 4)).copy()
    return xy, np.asarray(counts, dtype=np.int32), K, np.broadcast_to(np.stack((shear_pose(), still)), (8, 2, 4, 4)).copy()


@functools.lru_cache(maxsize=None)
def scene_case():
    """The first batch: lo_msac_ref.gpu_case() - B = 2, N = 768, counts 257 and 511, more rows than threads, no multiple of 256 -
    with the rows at and beyond the counts filled with NaN, and P = 3 poses per pair: the truth, one 5 degrees off (the scene's
    own start) and the truth with a NaN entry.  -> (xy, counts, intrinsics, poses (2, 3, 4, 4) fp32)."""
    xy, counts, K, _ = lm.gpu_case()
    xy = xy.copy()
    for b, c in enumerate(counts):
        xy[b, c:] = np.nan
    sc = lm.scene("curved")
    bad = rr.true_pose(sc)
    bad[1, 2] = np.nan
    poses = np.stack((rr.true_pose(sc), sc["rel_pose"], bad))
    return xy, counts, K, np.stack((poses, poses))


@functools.lru_cache(maxsize=None)
def want_stats(case):
    """residual_stats of every pair of scene_case ("scene") or shear_case ("shear") with Q_GPU and THR_GPU.  Shared."""
    xy, counts, K, poses = scene_case() if case == "scene" else shear_case()
    return [residual_stats(xy[b], counts[b], K[b], poses[b], Q_GPU, THR_GPU) for b in range(len(xy))]


ANGLES_DEG = (1e-6, 0.03, 1.0, 90.0, 179.9999)


@functools.lru_cache(maxsize=None)
def errors_case():
    """B = 3, P = 5 for cpn_pose_errors.  Pair 0: gt = [1 | (0.3, 0.1, -0.2)], the poses Rodrigues rotations by ANGLES_DEG about
    (0.3, 1, -0.2) - in fp32 the off-diagonal entries keep a 1e-6 degree turn to 2^-24 of itself - with translations 0, 180, 90
    and 1e-5 degrees from gt's direction and a zero vector.  Pair 1: a gt turned 40 degrees, the same turns times gt, translations
    of other lengths.  Pair 2: the truth itself, a NaN entry, an inf entry, a zero gt translation is pair 2's gt.
    -> (poses (3, 5, 4, 4) fp32, gt (3, 4, 4) fp32)."""
    axis = (0.3, 1.0, -0.2)
    gt = np.stack([np.eye(4)] * 3)
    gt[0, :3, 3] = (0.3, 0.1, -0.2)
    gt[1, :3, :3], gt[1, :3, 3] = mr.rodrigues((1.0, 0.2, 0.5), 40.0), (-0.5, 0.25, 1.5)
    gt[2, :3, :3] = mr.rodrigues((0.0, 1.0, 0.0), 10.0)
    poses = np.stack([np.stack([np.eye(4)] * 5)] * 3)
    side = np.cross(gt[0, :3, 3], (0.0, 0.0, 1.0))
    turns = (0.0, 180.0, 90.0, 1e-5)
    for p, deg in enumerate(ANGLES_DEG):
        poses[0, p, :3, :3] = mr.rodrigues(axis, deg)
        poses[0, p, :3, 3] = mr.rodrigues(side, turns[p]) @ gt[0, :3, 3] * (1.0 + p) if p < 4 else 0.0
        poses[1, p, :3, :3] = mr.rodrigues(axis, deg) @ gt[1, :3, :3]
        poses[1, p, :3, 3] = mr.rodrigues((0.0, 1.0, 0.0), 7.0 * p) @ gt[1, :3, 3] * (0.5 + p)
        poses[2, p, :3, :3] = mr.rodrigues(axis, 3.0 * p) @ gt[2, :3, :3]
        poses[2, p, :3, 3] = (0.1 * p, 0.2, 0.3)
    poses[2, 1, 0, 1], poses[2, 2, 2, 3] = np.nan, np.inf
    return poses.astype(np.float32), gt.astype(np.float32)
