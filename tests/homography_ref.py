"""Yardstick of coponerf_amd.matches.homography_pose (csrc/ransac_h.hip): a numpy restatement, for ONE pair and vectorised over the
hypotheses, of the three rules of include/coponerf_hip.h (round 22) in the header's operation sequence.  tests/test_homography_ref.py
holds it to independent forms on the CPU; tests/test_gpu_homography.py compares the kernels with it.  The sampler, the elimination,
the back substitution and the frames are tests/ransac_ref.py's, the Sampson rule tests/matches_ref.py's.

numpy float64 arithmetic is IEEE with one rounding per operation, which is what -ffp-contract=off gives the kernels, and every
expression below is written in the kernels' order: only + - * / sqrt and comparisons.  The decisions (the samples, the pivots, the
validity, the inliers, the winner, the votes, the pick) are integers or comparisons of values both sides form alike, so they are
compared exactly - after the fixtures have been shown to keep every transfer distance at least MARGIN = 1e-9 px from the threshold
and every m_2, w_2, N . b and determinant at least 1e-9 from 0.

Bounds (E = 2^-53), from operation counts, none from a run:
  null vector   rr.NULL_OPS E / (sigma_8 / sigma_1) per hypothesis, round 20's: the same elimination of an 8 x 9 system.
  the samples   |a x H b|_inf <= SAMPLE_OPS E kappa |a| |b| with kappa = sigma_1 / sigma_8 of the system and SAMPLE_OPS = 1000:
                the null vector's operations (under 700), the norm (18) and the product H b (15), generously.
  decomposition decompose_bound: DECOMP_OPS E max(1, 1 / (sigma_1^2 - sigma_3^2), 1 / (sigma_1 - 1), 1 / (1 - sigma_3)) (sigma_2 = 1)
                per entry of R, T and N.  8 sweeps of 3 rotations of about 30 operations, the norms, the two frames, u (12), the
                products and R (about 90), T (18): under 1000, DECOMP_OPS = 1000.  u_1,2 divide by sqrt(sigma_1^2 - sigma_3^2), and
                v_1 and v_3 are conditioned by the gaps of sigma_2 = 1 to sigma_1 and to sigma_3.
"""
import functools

import numpy as np

from tests import matches_ref as mr
from tests import ransac5_ref as r5
from tests import ransac_ref as rr

E = mr.E
CHUNK = rr.CHUNK
MARGIN = 1e-9
SAMPLE_OPS = 1000
DECOMP_OPS = 1000


# --------------------------------------------------------------------------------------------------------- the hypotheses
def adjugate(h, defect=None):
    """h (.., 9) -> adj(h) (.., 9) row-major, every entry one difference of two products.  defect="adjugate transposed"."""
    h = np.asarray(h, dtype=np.float64)
    g = np.stack((h[..., 4] * h[..., 8] - h[..., 5] * h[..., 7], h[..., 2] * h[..., 7] - h[..., 1] * h[..., 8],
                  h[..., 1] * h[..., 5] - h[..., 2] * h[..., 4], h[..., 5] * h[..., 6] - h[..., 3] * h[..., 8],
                  h[..., 0] * h[..., 8] - h[..., 2] * h[..., 6], h[..., 2] * h[..., 3] - h[..., 0] * h[..., 5],
                  h[..., 3] * h[..., 7] - h[..., 4] * h[..., 6], h[..., 1] * h[..., 6] - h[..., 0] * h[..., 7],
                  h[..., 0] * h[..., 4] - h[..., 1] * h[..., 3]), axis=-1)
    if defect == "adjugate transposed":
        g = g[..., [0, 3, 6, 1, 4, 7, 2, 5, 8]]
    return g


def determinant(h, g):
    return (h[..., 0] * g[..., 0] + h[..., 1] * g[..., 3]) + h[..., 2] * g[..., 6]


def third(M, p0, p1):
    return (M[..., 6] * p0 + M[..., 7] * p1) + M[..., 8]


def system(a0, a1, b0, b1):
    """(.., 4) each -> (.., 8, 9): match j gives rows 2 j = (b, 0, -a0 b) and 2 j + 1 = (0, b, -a1 b)."""
    one, zero = np.ones_like(a0), np.zeros_like(a0)
    with np.errstate(all="ignore"):
        top = np.stack((b0, b1, one, zero, zero, zero, -(a0 * b0), -(a0 * b1), -a0), axis=-1)
        bottom = np.stack((zero, zero, zero, b0, b1, one, -(a1 * b0), -(a1 * b1), -a1), axis=-1)
    return np.stack((top, bottom), axis=-2).reshape(a0.shape[:-1] + (8, 9))


def null_vector(A, defect=None):
    """A (H, 8, 9) -> (x (H, 9) the null vector with the last permuted unknown 1, valid (H) the rank test): round 20's."""
    A, perm, valid = rr.eliminate(A, 8, defect)
    return rr.back_substitute(A, perm, 8, free=8), valid


def hypotheses(xy, count, intrinsics, Hn, seed, defect=None):
    """The rule of cpn_ransac_homographies for one pair: xy (N, 4) fp32 -> (H (Hn, 9) float64, sample (Hn, 4) int32, valid (Hn)
    uint8, info: the systems, the determinants and the third components of the sample's points)."""
    xy = np.asarray(xy, dtype=np.float32)
    n = min(max(int(count), 0), len(xy))
    sample, got = rr.draw_samples(seed, Hn, n, defect=defect, k=4)
    k0, k1 = mr.cam_of(intrinsics[0]), mr.cam_of(intrinsics[1])
    rows = xy[np.maximum(sample, 0)]                                # (Hn, 4, 4)
    ok = (got == 4) & np.isfinite(rows).all(axis=(1, 2))
    a0, a1, b0, b1 = rr.normalised(rows, k0, k1)
    A = system(a0, a1, b0, b1)
    A[~ok] = 0.0
    with np.errstate(all="ignore"):
        x, valid = null_vector(A, defect)
        ss = x[:, 0] * x[:, 0]
        for c in range(1, 9):
            ss = ss + x[:, c] * x[:, c]
        h = x / np.sqrt(ss)[:, None]
        h = np.where((determinant(h, adjugate(h)) < 0.0)[:, None], -h, h)
        g = adjugate(h)
        det = determinant(h, g)
        m2 = third(h[:, None, :], b0, b1)                           # (Hn, 4)
        w2 = third(g[:, None, :], a0, a1)
        valid = valid & ok & (det > 0.0) & np.isfinite(det) & np.isfinite(h).all(axis=1)
        if defect != "no sample test":
            valid = valid & (m2 > 0.0).all(axis=1) & (w2 > 0.0).all(axis=1)
    h = np.where(valid[:, None], h, 0.0)
    return h, sample, valid.astype(np.uint8), {"A": A, "det": det, "m2": m2, "w2": w2, "ok": ok}


# ------------------------------------------------------------------------------------------------------------- the score
def transfer(M, fx, fy, p0, p1, q0, q1):
    """M (H, 9), points (n) -> (d (H, n) the distance in pixels of M p from q, third (H, n) the third component of M p)."""
    M = np.asarray(M, dtype=np.float64)[:, :, None]
    with np.errstate(all="ignore"):
        m0 = (M[:, 0] * p0 + M[:, 1] * p1) + M[:, 2]
        m1 = (M[:, 3] * p0 + M[:, 4] * p1) + M[:, 5]
        m2 = (M[:, 6] * p0 + M[:, 7] * p1) + M[:, 8]
        dx, dy = fx * (m0 / m2 - q0), fy * (m1 / m2 - q1)
        return np.sqrt(dx * dx + dy * dy), m2


def distances(Hm, xy, intrinsics, defect=None):
    """-> (d0, m2, d1, w2), each (H, n): the transfer distance and the third component in view 0 (by H) and view 1 (by adj H)."""
    k0, k1 = mr.cam_of(intrinsics[0]), mr.cam_of(intrinsics[1])
    a0, a1, b0, b1 = rr.normalised(xy, k0, k1)
    Hm = np.asarray(Hm, dtype=np.float64).reshape(-1, 9)
    d0, m2 = transfer(Hm, k0[0], k0[1], b0, b1, a0, a1)
    d1, w2 = transfer(adjugate(Hm, defect), k1[0], k1[1], a0, a1, b0, b1)
    return d0, m2, d1, w2


def inliers(Hm, xy, intrinsics, inlier_px, defect=None):
    """(H, n) bool: THE INLIER RULE.  defect="forward only": view 0's half alone; "no w2 test": w_2 > 0 is not asked;
    "adjugate transposed": adjugate's."""
    d0, m2, d1, w2 = distances(Hm, xy, intrinsics, defect)
    with np.errstate(invalid="ignore"):
        fwd = (m2 > 0.0) & np.isfinite(m2) & np.isfinite(d0) & (d0 <= inlier_px)
        back = np.isfinite(w2) & np.isfinite(d1) & (d1 <= inlier_px)
        if defect != "no w2 test":
            back &= w2 > 0.0
    return fwd if defect == "forward only" else fwd & back


def score(Hm, valid, xy, count, intrinsics, inlier_px, defect=None):
    """The rule of cpn_ransac_score_h for one pair -> partial (ceil(N / CHUNK), Hn) int32."""
    N, Hn = len(xy), len(Hm)
    n = min(max(int(count), 0), N)
    chunks = -(-N // CHUNK)
    inl = inliers(Hm, xy[:n], intrinsics, inlier_px, defect) & (np.asarray(valid) != 0)[:, None]
    padded = np.zeros((Hn, chunks * CHUNK), dtype=np.int32)
    padded[:, :n] = inl
    return np.ascontiguousarray(padded.reshape(Hn, chunks, CHUNK).sum(axis=2).T.astype(np.int32))


def threshold_margin(Hm, xy, intrinsics, inlier_px):
    """(the smallest | d - inlier_px | over both views' distances that are finite, the smallest |m_2| and |w_2|)."""
    d0, m2, d1, w2 = distances(Hm, xy, intrinsics)
    d = np.concatenate((d0.ravel(), d1.ravel()))
    z = np.concatenate((m2.ravel(), w2.ravel()))
    return float(np.abs(d[np.isfinite(d)] - inlier_px).min()), float(np.abs(z[np.isfinite(z)]).min())


# ------------------------------------------------------------------------------------------------------------- the finish
def jacobi(h):
    """Round 20's one-sided Jacobi method on G = h (9) with V = 1 and its ordering -> (G, V (3, 3), sg (3) descending)."""
    G, V = np.array(h, dtype=np.float64).reshape(3, 3), np.eye(3)
    with np.errstate(all="ignore"):
        for _ in range(rr.SWEEPS):
            for p, q in ((0, 1), (0, 2), (1, 2)):
                alpha = (G[0, p] * G[0, p] + G[1, p] * G[1, p]) + G[2, p] * G[2, p]
                beta = (G[0, q] * G[0, q] + G[1, q] * G[1, q]) + G[2, q] * G[2, q]
                gamma = (G[0, p] * G[0, q] + G[1, p] * G[1, q]) + G[2, p] * G[2, q]
                if gamma == 0.0:
                    continue
                zeta = (beta - alpha) / (2.0 * gamma)
                root = np.abs(zeta) + np.sqrt(1.0 + zeta * zeta)
                tt = (-1.0 if zeta < 0.0 else 1.0) / root
                c = 1.0 / np.sqrt(1.0 + tt * tt)
                s = c * tt
                for X in (G, V):
                    xp, xq = X[:, p].copy(), X[:, q].copy()
                    X[:, p] = c * xp - s * xq
                    X[:, q] = s * xp + c * xq
        sg = np.array([rr._norm3(G[:, c]) for c in range(3)])
        for p, q in ((0, 1), (1, 2), (0, 1)):
            if sg[p] < sg[q]:
                for X in (G, V):
                    X[:, [p, q]] = X[:, [q, p]]
                sg[[p, q]] = sg[[q, p]]
    return G, V, sg


def _matvec(M, x):
    return np.array([(M[i, 0] * x[0] + M[i, 1] * x[1]) + M[i, 2] * x[2] for i in range(3)])


def decompose(h, min_baseline=0.0):
    """The header's decomposition of a winner h (9) -> dict: s1, s3, Hs (3, 3), and either `Rn` (rotation only) or `R`, `T`,
    `N`: the lists of u_1's and u_2's (R, T, N) - candidate 2 k is (R[k], T[k], N[k]), candidate 2 k + 1 (R[k], -T[k], -N[k]) -,
    with `t` = T / |T| and `E` = [T]x R; `finite`."""
    h = np.asarray(h, dtype=np.float64)
    G, V, sg = jacobi(h)
    with np.errstate(all="ignore"):
        U, W = rr._frame(G), rr._frame(V)                           # rows u_k, v_k
        s1, s3 = sg[0] / sg[1], sg[2] / sg[1]
        Hs = (h / sg[1]).reshape(3, 3)
        out = {"s1": s1, "s3": s3, "Hs": Hs, "sg": sg}
        fin = bool(np.isfinite(s1) and np.isfinite(s3) and np.isfinite(Hs).all())
        gap = s1 * s1 - s3 * s3
        if not gap > 0.0 or s1 - s3 <= min_baseline:
            Rn = np.empty((3, 3))
            for i in range(3):
                for j in range(3):
                    Rn[i, j] = (U[0, i] * W[0, j] + U[1, i] * W[1, j]) + U[2, i] * W[2, j]
            out.update(Rn=Rn, finite=fin and bool(np.isfinite(Rn).all()))
            return out
        c1, c3 = 1.0 - s3 * s3, s1 * s1 - 1.0
        x1, x3, den = np.sqrt(c1 if c1 > 0.0 else 0.0), np.sqrt(c3 if c3 > 0.0 else 0.0), np.sqrt(gap)
        v2 = W[1]
        Rs, Ts, Ns, ts, Es = [], [], [], [], []
        for k in range(2):
            pa, pb = x1 * W[0], x3 * W[2]
            u = ((pa + pb) if k == 0 else (pa - pb)) / den
            Nv = rr._cross(v2, u)
            hv, hu = _matvec(Hs, v2), _matvec(Hs, u)
            hn = rr._cross(hv, hu)
            R = np.empty((3, 3))
            for i in range(3):
                for j in range(3):
                    R[i, j] = (hv[i] * v2[j] + hu[i] * u[j]) + hn[i] * Nv[j]
            T = np.array([((Hs[i, 0] - R[i, 0]) * Nv[0] + (Hs[i, 1] - R[i, 1]) * Nv[1]) + (Hs[i, 2] - R[i, 2]) * Nv[2] for i in range(3)])
            t = T / rr._norm3(T)
            fin = fin and bool(np.isfinite(R).all() and np.isfinite(t).all() and np.isfinite(Nv).all())
            Rs.append(R), Ts.append(T), Ns.append(Nv), ts.append(t), Es.append(mr.essential(R, T).reshape(9))
        out.update(R=Rs, T=Ts, N=Ns, t=ts, E=Es, finite=fin)
    return out


def decompose_bound(s1, s3):
    with np.errstate(all="ignore"):
        return DECOMP_OPS * E * max(1.0, 1.0 / (s1 * s1 - s3 * s3), 1.0 / (s1 - 1.0), 1.0 / (1.0 - s3))


def candidates(dec):
    """The four (R, T, N) of a decomposition in the header's order."""
    out = []
    for k in range(2):
        out += [(dec["R"][k], dec["T"][k], dec["N"][k]), (dec["R"][k], -dec["T"][k], -dec["N"][k])]
    return out


def finish(Hm, valid, partial, xy, count, intrinsics, inlier_px, rel_pose=None, min_baseline=0.0, defect=None):
    """The rule of cpn_ransac_finish_h for one pair -> (pose, twin (4, 4) float64 before the fp32 store, Hout (9), inlier (N)
    uint8, stats (12), info).  defect="last on ties": the higher index wins a tie; "vote on a": the vote asks N . a;
    "twins swapped": pose and twin change places."""
    xy = np.asarray(xy, dtype=np.float32)
    N, Hn = len(xy), len(Hm)
    n = min(max(int(count), 0), N)
    usable = int(np.isfinite(xy[:n]).all(axis=1).sum())
    used = -(-n // CHUNK)
    inlier = np.zeros(N, dtype=np.uint8)
    stats = np.zeros(12)
    nothing = usable < 4 or Hn == 0
    ok = np.asarray(valid) != 0
    sums = np.asarray(partial)[:used].sum(axis=0, dtype=np.int64) if Hn else np.zeros(0, dtype=np.int64)
    info = {"sums": sums}
    dec = None
    if not nothing and ok.any():
        cand = np.where(ok, sums, -1)
        winner = int(len(cand) - 1 - cand[::-1].argmax()) if defect == "last on ties" else int(cand.argmax())
        dec = decompose(Hm[winner], min_baseline)
    if nothing or dec is None or not dec["finite"]:
        pose = np.eye(4) if rel_pose is None else np.asarray(rel_pose, dtype=np.float32).astype(np.float64)
        stats[1] = 0.0 if nothing else usable
        stats[11] = 2.0 if nothing else 1.0
        return pose, pose.copy(), np.zeros(9), inlier, stats, info
    k0, k1 = mr.cam_of(intrinsics[0]), mr.cam_of(intrinsics[1])
    inl = inliers(Hm[winner][None], xy[:n], intrinsics, inlier_px)[0]
    inlier[:n] = inl
    stats[:4] = float(sums[winner]), float(usable), float(winner), float(ok.sum())
    stats[8], stats[9], stats[10] = dec["s1"], dec["s3"], dec["s1"] - dec["s3"]
    info.update(winner=winner, dec=dec)
    pose = np.eye(4)
    if "Rn" in dec:
        pose[:3, :3] = dec["Rn"]
        stats[11] = 3.0
        return pose, pose.copy(), dec["Hs"].reshape(9), inlier, stats, info
    a0, a1, b0, b1 = rr.normalised(xy[:n], k0, k1)
    votes, samp, small = [], [], np.inf
    for k in range(2):
        Nv = dec["N"][k]
        p0, p1 = (a0, a1) if defect == "vote on a" else (b0, b1)
        nb = ((Nv[0] * p0 + Nv[1] * p1) + Nv[2])[inl]
        if len(nb):
            small = min(small, float(np.abs(nb).min()))
        votes += [int((nb > 0.0).sum()), int((nb < 0.0).sum())]
        samp.append(int(rr.inliers(dec["E"][k][None], xy[:n], intrinsics, inlier_px)[0].sum()))
    pick = 0
    for c in range(1, 4):
        if votes[c] > votes[pick] or (votes[c] == votes[pick] and samp[c >> 1] > samp[pick >> 1]):
            pick = c
    other = 1 - (pick >> 1)
    tw = 2 * other + 1 if votes[2 * other + 1] > votes[2 * other] else 2 * other
    if defect == "twins swapped":
        pick, tw, other = tw, pick, pick >> 1
    _, _, len0, rel_ok = rr.rel_parts(rel_pose)
    twin = np.eye(4)
    for P, c in ((pose, pick), (twin, tw)):
        P[:3, :3], P[:3, 3] = dec["R"][c >> 1], (len0 if rel_ok else 1.0) * ((-1.0 if c & 1 else 1.0) * dec["t"][c >> 1])
    stats[4:8] = votes[pick], votes[tw], samp[pick >> 1], samp[other]
    info.update(votes=np.array(votes), samp=np.array(samp), pick=pick, twin=tw, small_nb=small)
    return pose, twin, dec["Hs"].reshape(9), inlier, stats, info


def homography_pose(xy, count, intrinsics, rel_pose=None, hypotheses_n=1024, inlier_px=1.0, seed=0, min_baseline=0.0, defect=None):
    """The three rules in a row for one pair -> (pose, twin, Hout, inlier, stats, info); info also holds H, sample, valid, partial."""
    Hm, sample, valid, _ = hypotheses(xy, count, intrinsics, hypotheses_n, seed, defect)
    partial = score(Hm, valid, xy, count, intrinsics, inlier_px, defect)
    pose, twin, Hout, inlier, stats, info = finish(Hm, valid, partial, xy, count, intrinsics, inlier_px, rel_pose, min_baseline, defect)
    info.update(H=Hm, sample=sample, valid=valid, partial=partial)
    return pose, twin, Hout, inlier, stats, info


# ------------------------------------------------------------------------------------------------------------- the scenes
CURVED = dict(n=1000, seed=16, noise_px=0.5, outliers=0.3)
NAN_ROW = 17
MIN_BASELINE = 0.05                # between the rotation scene's sigma_1 - sigma_3 and the wall's


@functools.lru_cache(maxsize=None)
def rotation_scene(n=1000, seed=16, noise_px=0.5, outliers=0.3):
    """refine_scene with t = 0: the same cameras, rotation and random stream.  Returns refine_scene's dict (t_true is 0)."""
    rng = np.random.default_rng(seed)
    S, f = 256, 200.0
    R_true, t_true = mr.rodrigues((0.3, 1.0, -0.2), 12.0), np.zeros(3)
    p0 = rng.uniform(0.0, S, size=(n, 2))
    depth = rng.uniform(1.0, 6.0, size=n)
    X0 = np.concatenate(((p0 - S / 2.0) / f, np.ones((n, 1))), 1) * depth[:, None]
    X1 = (X0 - t_true) @ R_true
    p1 = f * X1[:, :2] / X1[:, 2:] + S / 2.0
    if noise_px:
        p1 = p1 + rng.normal(scale=noise_px, size=p1.shape)
    if outliers:
        bad = rng.random(n) < outliers
        p1[bad] = rng.uniform(0.0, S, size=(int(bad.sum()), 2))
    K = mr.pinhole(f, S)
    return {"xy": np.concatenate((p0, p1), 1).astype(np.float32), "intrinsics": np.stack((K, K)),
            "rel_pose": mr.refine_scene()["rel_pose"], "R_true": R_true, "t_true": t_true}


def scenes():
    """(name, scene) of the three scenes: the wall, the curved scene and the pure rotation."""
    return (("wall", r5.wall_scene(**r5.WALL)), ("curved", mr.refine_scene(**CURVED)), ("rotation", rotation_scene()))


@functools.lru_cache(maxsize=None)
def scene_result(name, hypotheses_n=1024, seed=0, min_baseline=0.0):
    sc = dict(scenes())[name]
    return sc, homography_pose(sc["xy"], 1000, sc["intrinsics"], rr.true_pose(sc) if name != "rotation" else None, hypotheses_n, 1.0,
                               seed, min_baseline)


def collinear_rows():
    """Six matches of a shift by (11, 16) pixels at integer pixels; the first three lie on one line in each image (y constant):
    exactly collinear in float64, and any four of the six that do not hold all three determine the shift."""
    p0 = np.array([[20.0, 64.0], [90.0, 64.0], [200.0, 64.0], [40.0, 150.0], [180.0, 30.0], [120.0, 220.0]])
    return np.concatenate((p0, p0 + (11.0, 16.0)), 1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def hypotheses_case():
    """B = 6 pairs of N = 100 rows of the wall: counts 64 with a NaN row in reach of the sampler, 6 (redraws; collinear_rows: rows
    0, 1, 2 are three collinear points), 4 (every sample is the same four rows), 1000 (beyond N) whose rows 0 .. 49 are copies of one
    match, -3, and 3 (below 4).  -> (xy (6, 100, 4) fp32, counts (6) int32, intrinsics (6, 2, 4, 4) fp32).  Shared, never
    written to."""
    sc = r5.wall_scene(**r5.WALL)
    xy = np.stack([sc["xy"][100 * b:100 * b + 100] for b in (0, 1, 2, 3, 4, 5)]).copy()
    xy[0, NAN_ROW, 2] = np.nan
    xy[1, :6] = collinear_rows()
    xy[3, :50] = xy[3, 50]
    return xy, np.asarray((64, 6, 4, 1000, -3, 3), dtype=np.int32), np.stack([sc["intrinsics"]] * 6)


@functools.lru_cache(maxsize=None)
def score_case(Hn=257):
    """B = 3 pairs of N = 2 CHUNK + 3 rows of the wall (three chunks, the last of three rows), counts (N, 0, CHUNK + 7); H and valid
    are the restatement's own hypotheses of pair 0 for every pair, every seventh hypothesis and hypothesis 255 switched off on top
    of the ones that are invalid by themselves; hypothesis 256, alone in the second tile, is valid.
    -> (xy, counts, intrinsics, H (3, Hn, 9), valid (3, Hn))."""
    sc = r5.wall_scene(**r5.WALL)
    N = 2 * CHUNK + 3
    xy = np.stack([sc["xy"][:N]] * 3).copy()
    Hm, _, valid, _ = hypotheses(xy[0], N, sc["intrinsics"], Hn, 0)
    Hm, valid = Hm.copy(), valid.copy()
    Hm[256], valid[256] = Hm[np.flatnonzero(valid)[1]], 1           # whatever the draw gave slot 256: a copy of a valid one
    valid[::7] = 0
    valid[255] = 0
    return xy, np.asarray((N, 0, CHUNK + 7), dtype=np.int32), np.stack([sc["intrinsics"]] * 3), np.stack([Hm] * 3), np.stack([valid] * 3)


FINISH_PAIRS = ("wall", "curved", "rotation", "tie", "invalid", "few", "identity")


@functools.lru_cache(maxsize=None)
def finish_case(Hn=64):
    """B = 7 pairs of N = 1000 rows, Hn = 64: the three scenes; the wall with its winner copied into a later slot (a tie that the
    lower index must win); the wall with every hypothesis invalid (status 1); the wall with count 3 (status 2); and matches that
    do not move with H = 1 / sqrt(3) in every valid slot (status 3 at any min_baseline).  rel_pose is the stalled start of the
    curved scene.  -> (xy, counts, intrinsics, rel_pose, H, valid, partial (7, chunks, Hn) int32), the last three the
    restatement's."""
    named = dict(scenes())
    wall = named["wall"]
    still = wall["xy"].copy()
    still[:, 2:] = still[:, :2]
    xy = np.stack((wall["xy"], named["curved"]["xy"], named["rotation"]["xy"], wall["xy"], wall["xy"], wall["xy"], still))
    counts = np.asarray((1000, 1000, 1000, 1000, 1000, 3, 1000), dtype=np.int32)
    K = np.stack([wall["intrinsics"]] * 7)
    P = np.stack([rr.stalled_start(named["curved"])] * 7)
    Hs, vs, ps = [], [], []
    for b, name in enumerate(FINISH_PAIRS):
        Hm, _, valid, _ = hypotheses(xy[b], counts[b], K[b], Hn, 0)
        valid = valid.copy()
        if name == "tie":
            sums = score(Hm, valid, xy[b], counts[b], K[b], 1.0).sum(axis=0)
            w = int(np.where(valid != 0, sums, -1).argmax())
            Hm = Hm.copy()
            Hm[(w + 7) % Hn], valid[(w + 7) % Hn] = Hm[w], 1
        if name == "invalid":
            valid[:] = 0
        if name == "identity":
            Hm = np.where((valid != 0)[:, None], (np.eye(3) / np.sqrt(3.0)).reshape(9)[None], 0.0)
        Hs.append(Hm)
        vs.append(valid)
        ps.append(score(Hm, valid, xy[b], counts[b], K[b], 1.0))
    return xy, counts, K, P, np.stack(Hs), np.stack(vs), np.stack(ps)
