"""Yardstick of coponerf_amd.triangulate.bundle_adjust (csrc/bundle.hip, round 27 of include/coponerf_hip.h): a numpy float64
restatement of cpn_bundle_adjust, operation by operation, for ONE pair.  tests/test_bundle_ref.py pins it on the CPU against forms it
shares no code with (central differences, the full (6 + 3 n)-square normal equations, a dense gauge-constrained inverse, round 26's
points, a Monte-Carlo); tests/test_gpu_bundle.py compares the kernel with it.

The 30 sums are tests/matches_ref.py's block_sum (thread t adds the rows t, t + 256, .. in ascending order, the butterfly, then
(w0 + w1) + (w2 + w3)), the 6 x 6 solve its solve6, the step its apply_step; the 3 x 3 inverses are chol_solve below, the same
Cholesky for any size, over all rows at once.  numpy float64 arithmetic is IEEE, one rounding per operation, which is what
-ffp-contract=off gives the kernel: where only + - x / sqrt are used (iters = 0) the outputs are compared in their bits; a step takes
the device library's sin and cos, so across steps bounds are used (step_bound).

defect= seeds a wrong rule, which the CPU tests must catch: "no len" (the tentative points are not divided by |t + dt|), "stale
lambda" (a rejection leaves lambda as it is), "backsub sign" (dX = +Vi v), "no gauge" (C is the inverse alone, without - u u^T / p).
The weight's derivative is not taken anywhere in the rule, so there is no frozen-derivative defect to seed.
"""
import functools

import numpy as np

from tests import matches_ref as mr
from tests import triangulate_ref as tr

MARGIN = 1e-9
DEG = 57.29577951308232
LAMBDA0, UP, DOWN, LAMBDA_MIN, LAMBDA_MAX = 1e-3, 4.0, 3.0, 1e-12, 1e8
DEFECTS = ("no len", "stale lambda", "backsub sign", "no gauge")
E = 2.0 ** -53


def residual(R, t, k0, k1, X, m, s2):
    """The header's residual of the rows X (n, 3), m (n, 4) at (R, t) -> dict of d, Y (lists of 3 arrays), r (list of 4), e2, cost, w."""
    d = [X[:, j] - t[j] for j in range(3)]
    Y = [(R[0, j] * d[0] + R[1, j] * d[1]) + R[2, j] * d[2] for j in range(3)]
    p = [(k0[0] * X[:, 0]) / X[:, 2] + k0[2], (k0[1] * X[:, 1]) / X[:, 2] + k0[3], (k1[0] * Y[0]) / Y[2] + k1[2], (k1[1] * Y[1]) / Y[2] + k1[3]]
    r = [p[a] - m[:, a] for a in range(4)]
    e2 = ((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]) + r[3] * r[3]
    u = 1.0 + e2 / s2
    return {"d": d, "Y": Y, "r": r, "e2": e2, "cost": (e2 / 2.0) / u, "w": 1.0 / (u * u)}


def jacobians(R, k0, k1, X, q):
    """(Jx [4][3], Jp [2][6]) of the rows, lists of arrays: J_x = [A; M], the last two rows of J_p = [M [d]x, -M]."""
    zero = np.zeros(len(X))
    x0, x1, x2 = X[:, 0], X[:, 1], X[:, 2]
    Y, d = q["Y"], q["d"]
    Jx = [[k0[0] / x2, zero, -(((k0[0] * x0) / x2) / x2)], [zero, k0[1] / x2, -(((k0[1] * x1) / x2) / x2)]]
    P = [[k1[0] / Y[2], zero, -(((k1[0] * Y[0]) / Y[2]) / Y[2])], [zero, k1[1] / Y[2], -(((k1[1] * Y[1]) / Y[2]) / Y[2])]]
    Jp = []
    for a in range(2):
        M = [(P[a][0] * R[c, 0] + P[a][1] * R[c, 1]) + P[a][2] * R[c, 2] for c in range(3)]
        Jx.append(M)
        Jp.append([M[1] * d[2] - M[2] * d[1], M[2] * d[0] - M[0] * d[2], M[0] * d[1] - M[1] * d[0], -M[0], -M[1], -M[2]])
    return Jx, Jp


def blocks(R, k0, k1, X, q, lam):
    """The row's blocks -> dict: V (n, 3, 3) with its diagonal damped, W (n, 6, 3), gx (n, 3), U (n, 21), gp (n, 6), Jx, Jp."""
    Jx, Jp = jacobians(R, k0, k1, X, q)
    w, r, n = q["w"], q["r"], len(X)
    wJx = [[w * Jx[a][c] for c in range(3)] for a in range(4)]
    wJp = [[w * Jp[a][j] for j in range(6)] for a in range(2)]
    V, gx = np.empty((n, 3, 3)), np.empty((n, 3))
    for c in range(3):
        for k in range(c, 3):
            V[:, c, k] = V[:, k, c] = ((wJx[0][c] * Jx[0][k] + wJx[1][c] * Jx[1][k]) + wJx[2][c] * Jx[2][k]) + wJx[3][c] * Jx[3][k]
        gx[:, c] = ((wJx[0][c] * r[0] + wJx[1][c] * r[1]) + wJx[2][c] * r[2]) + wJx[3][c] * r[3]
    for c in range(3):
        V[:, c, c] = V[:, c, c] + lam * V[:, c, c]
    W, U, gp = np.empty((n, 6, 3)), np.empty((n, 21)), np.empty((n, 6))
    at = 0
    for j in range(6):
        for c in range(3):
            W[:, j, c] = wJp[0][j] * Jx[2][c] + wJp[1][j] * Jx[3][c]
        for k in range(j, 6):
            U[:, at] = wJp[0][j] * Jp[0][k] + wJp[1][j] * Jp[1][k]
            at += 1
        gp[:, j] = wJp[0][j] * r[2] + wJp[1][j] * r[3]
    return {"V": V, "W": W, "gx": gx, "U": U, "gp": gp, "Jx": Jx, "Jp": Jp}


def chol_solve(A, g):
    """cholesky_solve.h for a stack: A (n, p, p), g (n, p) -> (x = -A^-1 g (n, p), ok (n)): a pivot that is not positive or not
    finite, or an x that is not finite, fails the row (its x is then not used)."""
    L = A.copy()
    n, p = g.shape
    ok = np.ones(n, dtype=bool)
    with np.errstate(all="ignore"):
        for j in range(p):
            s = L[:, j, j].copy()
            for k in range(j):
                s = s - L[:, j, k] * L[:, j, k]
            ok &= (s > 0.0) & np.isfinite(s)
            l = np.sqrt(s)
            L[:, j, j] = l
            for i in range(j + 1, p):
                v = L[:, i, j].copy()
                for k in range(j):
                    v = v - L[:, i, k] * L[:, j, k]
                L[:, i, j] = v / l
        y, x = np.zeros((n, p)), np.zeros((n, p))
        for i in range(p):
            v = -g[:, i]
            for k in range(i):
                v = v - L[:, i, k] * y[:, k]
            y[:, i] = v / L[:, i, i]
        for i in range(p - 1, -1, -1):
            v = y[:, i].copy()
            for k in range(i + 1, p):
                v = v - L[:, k, i] * x[:, k]
            x[:, i] = v / L[:, i, i]
        ok &= np.isfinite(x).all(axis=1)
    return x, ok


def inverse(V):
    """(Vi (n, p, p), ok (n)): column k of the inverse by chol_solve with the right side -e_k."""
    n, p = V.shape[:2]
    Vi, ok = np.empty_like(V), np.ones(n, dtype=bool)
    for k in range(p):
        g = np.zeros((n, p))
        g[:, k] = -1.0
        x, good = chol_solve(V, g)
        Vi[:, :, k] = x
        ok &= good
    return Vi, ok


def times_inverse(W, Vi):
    """T = W Vi, (n, 6, 3)."""
    T = np.empty_like(W)
    for j in range(6):
        for c in range(3):
            T[:, j, c] = (W[:, j, 0] * Vi[:, 0, c] + W[:, j, 1] * Vi[:, 1, c]) + W[:, j, 2] * Vi[:, 2, c]
    return T


def _scatter(n, on, values):
    out = np.zeros((n,) + values.shape[1:])
    out[on] = values
    return out


def sweep_a(R, t, k0, k1, X, m, on, s2, lam):
    """The 30 sums of sweep A at the kept state over the rows below the count (X (n, 3), m (n, 4), on (n) bool: the used rows)."""
    n = len(X)
    with np.errstate(all="ignore"):
        q = residual(R, t, k0, k1, X[on], m[on], s2)
        bl = blocks(R, k0, k1, X[on], q, lam)
        Vi, ok = inverse(bl["V"])
        T = times_inverse(bl["W"], Vi)
        W, gx = bl["W"], bl["gx"]
        cols, at = [], 0
        for j in range(6):
            for k in range(j, 6):
                cols.append(bl["U"][:, at] - ((T[:, j, 0] * W[:, k, 0] + T[:, j, 1] * W[:, k, 1]) + T[:, j, 2] * W[:, k, 2]))
                at += 1
        for j in range(6):
            cols.append(bl["gp"][:, j] - ((T[:, j, 0] * gx[:, 0] + T[:, j, 1] * gx[:, 1]) + T[:, j, 2] * gx[:, 2]))
        terms = np.where(ok[:, None], np.stack(cols, 1), 0.0)
        terms = np.concatenate((terms, np.stack((q["cost"], q["w"], np.ones(len(ok))), 1)), 1)
    return mr.block_sum(_scatter(n, on, terms))


def reduced(sums, t, lam):
    """(A, g, S, pin) of the solve: S the symmetric matrix of the sums, pin = tr S / 6, A = S with A_jj = S_jj + lam S_jj (lam
    None: no damping, the covariance's form) and the translation block += pin t t^T."""
    S = np.zeros((6, 6))
    at = 0
    for j in range(6):
        for k in range(j, 6):
            S[j, k] = S[k, j] = sums[at]
            at += 1
    trace = 0.0
    for j in range(6):
        trace += S[j, j]
    pin = trace / 6.0
    A = S.copy()
    if lam is not None:
        for j in range(6):
            A[j, j] = S[j, j] + lam * S[j, j]
    for i in range(3):
        for j in range(3):
            A[3 + i, 3 + j] = A[3 + i, 3 + j] + pin * (t[i] * t[j])
    return A, sums[21:27].copy(), S, pin


def back_substitute(R, t, k0, k1, X, m, s2, lam, delta, defect=None):
    """dX (n, 3) of the used rows X at the kept state for the reduced step delta; 0 where the row's solves fail."""
    with np.errstate(all="ignore"):
        q = residual(R, t, k0, k1, X, m, s2)
        bl = blocks(R, k0, k1, X, q, lam)
        Vi, ok = inverse(bl["V"])
        W, gx = bl["W"], bl["gx"]
        v = [gx[:, c] + (((((W[:, 0, c] * delta[0] + W[:, 1, c] * delta[1]) + W[:, 2, c] * delta[2]) + W[:, 3, c] * delta[3]) +
                          W[:, 4, c] * delta[4]) + W[:, 5, c] * delta[5]) for c in range(3)]
        dX = np.stack([-((Vi[:, a, 0] * v[0] + Vi[:, a, 1] * v[1]) + Vi[:, a, 2] * v[2]) for a in range(3)], 1)
        if defect == "backsub sign":
            dX = -dX
    return np.where(ok[:, None], dX, 0.0)


def sweep_b(R, t, Rn, tn, ln, k0, k1, X, m, on, s2, lam, delta, defect=None):
    """(X' (n, 3), the trial cost, the smallest |depth| the test of X' saw) of sweep B."""
    n = len(X)
    Xn = np.full((n, 3), np.nan)
    with np.errstate(all="ignore"):
        dX = back_substitute(R, t, k0, k1, X[on], m[on], s2, lam, delta, defect)
        Xn[on] = (X[on] + dX) if defect == "no len" else (X[on] + dX) / ln
        qn = residual(Rn, tn, k0, k1, Xn[on], m[on], s2)
        good = np.isfinite(Xn[on]).all(axis=1) & (Xn[on][:, 2] > 0.0) & (qn["Y"][2] > 0.0)
        cost = mr.block_sum(_scatter(n, on, np.where(good, qn["cost"], 0.0)[:, None]))[0]
        depth = float(np.min(np.abs(np.concatenate((Xn[on][:, 2], qn["Y"][2]))))) if on.any() else np.inf
    return Xn, (cost if good.all() else np.inf), depth


def start(xy, count, intrinsics, pose, xyz_in, flag, inlier, s2, pose64=None):
    """The state the kernel starts from (pose64: a float64 pose to start from instead of pose's fp32 values - for the CPU tests
    alone, as triangulate_ref.rows64 takes float64 coordinates: an fp32 rotation is orthonormal to 6e-8 only, the rule never
    re-orthonormalises it, and R^T (X - t) then differs from the inverse of R X + t by as much) -> None where the pose or the cameras are not usable, else dict of R, t, len0, k0, k1, m
    (n, 4), X (n, 3) (NaN where not used), on (n) bool, depth: the smallest |X_2|, |Y_2| of the rows that reach that test."""
    P = np.asarray(pose, dtype=np.float32).astype(np.float64) if pose64 is None else np.asarray(pose64, dtype=np.float64)
    k0, k1 = mr.cam_of(intrinsics[0]), mr.cam_of(intrinsics[1])
    R, t0 = P[:3, :3].copy(), P[:3, 3].copy()
    with np.errstate(all="ignore"):
        len0 = np.sqrt((t0[0] * t0[0] + t0[1] * t0[1]) + t0[2] * t0[2])
    if not (np.isfinite(R).all() and np.isfinite(t0).all() and len0 > 0.0 and np.isfinite(len0) and np.isfinite(k0 + k1).all()):
        return None
    xy32 = np.asarray(xy, dtype=np.float32)
    n = min(max(int(count), 0), len(xy32))
    m = xy32[:n].astype(np.float64)
    t = t0 / len0
    with np.errstate(all="ignore"):
        X = np.asarray(xyz_in, dtype=np.float32)[:n].astype(np.float64) / len0
        on = np.isfinite(m).all(axis=1) & (np.asarray(flag)[:n] == 0) & np.isfinite(X).all(axis=1)
        if inlier is not None:
            on &= np.asarray(inlier)[:n] != 0
        q = residual(R, t, k0, k1, X, m, s2)
        depth = np.concatenate((X[on][:, 2], q["Y"][2][on]))
        on &= (X[:, 2] > 0.0) & (q["Y"][2] > 0.0)
    X = np.where(on[:, None], X, np.nan)
    return {"R": R, "t": t, "len0": len0, "k0": k0, "k1": k1, "m": m, "X": X, "on": on, "P": P,
            "depth": float(np.abs(depth).min()) if len(depth) else np.inf}


def covariance(sums, t, defect=None):
    """C (6, 6) of the last sweep A's sums (lambda = 0), or None where a solve fails."""
    A, _, S, pin = reduced(sums, t, None)
    C, ok = inverse(A[None])
    if not ok[0]:
        return None
    C = C[0]
    if defect != "no gauge":
        for i in range(3):
            for j in range(3):
                C[3 + i, 3 + j] = C[3 + i, 3 + j] - (t[i] * t[j]) / pin
    return C


def point_covariances(R, t, k0, k1, X, m, s2, C):
    """(Cov (n, 6): the upper triangle of Vi + T^T C T at lambda = 0, NaN where the row's solves fail; q: the residual's dict)."""
    with np.errstate(all="ignore"):
        q = residual(R, t, k0, k1, X, m, s2)
        bl = blocks(R, k0, k1, X, q, 0.0)
        Vi, ok = inverse(bl["V"])
        T = times_inverse(bl["W"], Vi)
        CT = np.empty_like(T)
        for j in range(6):
            for c in range(3):
                CT[:, j, c] = ((((C[j, 0] * T[:, 0, c] + C[j, 1] * T[:, 1, c]) + C[j, 2] * T[:, 2, c]) + C[j, 3] * T[:, 3, c]) +
                               C[j, 4] * T[:, 4, c]) + C[j, 5] * T[:, 5, c]
        cols = []
        for a in range(3):
            for c in range(a, 3):
                cols.append(Vi[:, a, c] + (((((T[:, 0, a] * CT[:, 0, c] + T[:, 1, a] * CT[:, 1, c]) + T[:, 2, a] * CT[:, 2, c]) +
                                             T[:, 3, a] * CT[:, 3, c]) + T[:, 4, a] * CT[:, 4, c]) + T[:, 5, a] * CT[:, 5, c]))
    return np.where(ok[:, None], np.stack(cols, 1), np.nan), q


def bundle_adjust(xy, count, intrinsics, pose, xyz_in, flag, inlier=None, iters=10, scale_px=1.0, ftol=1e-12, min_rows=8, defect=None,
                  perturb=None, pose64=None):
    """The rule of cpn_bundle_adjust for ONE pair: xy (N, 4) fp32, count, intrinsics (2, 4, 4), pose (4, 4) fp32, xyz_in (N, 3) fp32
    and flag (N) uint8 (cpn_triangulate_matches' under that pose), inlier None or (N) uint8 -> dict of the kernel's outputs `pose`
    (4, 4) fp32, `xyz` (N, 3) fp32, `geom` (N, 4) fp32, `cov_x` (N, 6) fp32, `cov` (6, 6), `stats` (12); the float64 values before
    the fp32 stores `pose64`, `xyz64`, `geom64`, `cov_x64`; `X` (N, 3) the points under |t| = 1; `R`, `t`; and `trace`: per solve
    the dict of lam, kept, trial, accepted, delta, A, g, len, the state it was formed at, the depth margin of sweep B; `depth` the
    smallest |depth| any in-front test saw.  perturb = (k, v): v (6) is added to the reduced step of solve k - what output_bounds
    differentiates by; never part of the rule.  pose64: start()'s, for the CPU tests alone."""
    N = len(xy)
    s2 = float(scale_px) * float(scale_px)
    out = {"pose": np.asarray(pose, dtype=np.float32).copy(), "xyz": np.full((N, 3), np.nan, dtype=np.float32),
           "geom": np.full((N, 4), np.nan, dtype=np.float32), "cov_x": np.full((N, 6), np.nan, dtype=np.float32), "cov": np.full((6, 6), np.nan),
           "trace": [], "depth": np.inf}
    st = start(xy, count, intrinsics, pose, xyz_in, flag, inlier, s2, pose64)
    n_used = 0 if st is None else int(st["on"].sum())
    if st is None or n_used < min_rows:
        stats = np.full(12, np.nan)
        stats[3], stats[4], stats[5], stats[11] = float(n_used), 0.0, 0.0, 2.0
        out["stats"] = stats
        return out
    R, t, len0, k0, k1, m, X, on = (st[k] for k in ("R", "t", "len0", "k0", "k1", "m", "X", "on"))
    n = len(m)
    lam, final = LAMBDA0, iters == 0
    accepted = rejected = solves = status = 0
    cost0, depth, trace = None, st["depth"], []
    while True:
        sums = sweep_a(R, t, k0, k1, X, m, on, s2, 0.0 if final else lam)
        kept = sums[27]
        if cost0 is None:
            cost0 = kept
        if final:
            break
        A, g, S, pin = reduced(sums, t, lam)
        delta = mr.solve6(A, g)
        new = None
        if delta is not None and perturb is not None and perturb[0] == solves:
            delta = delta + perturb[1]
        if delta is not None:
            tn = t + delta[3:]
            ln = np.sqrt((tn[0] * tn[0] + tn[1] * tn[1]) + tn[2] * tn[2])
            new = mr.apply_step(R, t, delta)
        if new is None:
            status, final = 1, True
            continue
        solves += 1
        Xn, trial, dz = sweep_b(R, t, new[0], new[1], ln, k0, k1, X, m, on, s2, lam, delta, defect)
        depth = min(depth, dz)
        step = {"lam": lam, "kept": kept, "trial": trial, "accepted": bool(trial < kept), "delta": delta, "A": A, "g": g, "S": S, "len": ln,
                "R": R, "t": t, "X": X, "sums": sums, "depth": dz}
        trace.append(step)
        if trial < kept:
            accepted += 1
            R, t, X = new[0], new[1], Xn
            lam = max(lam / DOWN, LAMBDA_MIN)
            step["stop"] = (kept - trial) / (ftol * kept) if ftol * kept > 0.0 else np.inf   # <= 1 stops
            if kept - trial <= ftol * kept:
                final = True
        else:
            rejected += 1
            if defect != "stale lambda":
                lam = UP * lam
            step["stop"] = lam / LAMBDA_MAX                                                  # > 1 stops
            if lam > LAMBDA_MAX:
                final = True
        if solves >= iters:
            final = True
    C = covariance(sums, t, defect)
    if C is None:
        status, C = 1, np.full((6, 6), np.nan)
    with np.errstate(all="ignore"):
        Cov, q = point_covariances(R, t, k0, k1, X[on], m[on], s2, C)
        rows = sums[29]
        sigma = np.sqrt((2.0 * kept) / (rows - 5.0)) if rows > 5.0 else np.nan
        dR = 0.0
        for r in range(3):
            for c in range(3):
                e = R[r, c] - st["P"][r, c]
                dR += e * e
        moved = 2.0 * np.arcsin(min(np.sqrt(dR) / 2.8284271247461903, 1.0)) * DEG
        stats = np.array([cost0, kept, sums[28], rows, float(accepted), float(rejected), lam, sigma,
                          (sigma * np.sqrt((C[0, 0] + C[1, 1]) + C[2, 2])) * DEG, (sigma * np.sqrt((C[3, 3] + C[4, 4]) + C[5, 5])) * DEG, moved,
                          float(status)])
        pose64 = np.eye(4)
        pose64[:3, :3], pose64[:3, 3] = R, len0 * t
        xyz64, geom64, cov64 = np.full((N, 3), np.nan), np.full((N, 4), np.nan), np.full((N, 6), np.nan)
        rows_on = np.flatnonzero(on)
        xyz64[rows_on] = len0 * X[on]
        geom64[rows_on] = np.stack((len0 * X[on][:, 2], len0 * q["Y"][2], np.sqrt(q["e2"]), q["w"]), 1)
        cov64[rows_on] = (len0 * len0) * Cov
        out.update({"pose": pose64.astype(np.float32), "pose64": pose64, "xyz": xyz64.astype(np.float32), "xyz64": xyz64,
                    "geom": geom64.astype(np.float32), "geom64": geom64, "cov_x": cov64.astype(np.float32), "cov_x64": cov64, "cov": C,
                    "stats": stats, "trace": trace, "depth": depth, "R": R, "t": t, "len0": len0,
                    "X": np.concatenate((X, np.full((N - n, 3), np.nan))), "on": np.concatenate((on, np.zeros(N - n, dtype=bool))),
                    "sums": sums, "k0": k0, "k1": k1, "m": m, "s2": s2})
    return out


def margins(res):
    """The smallest relative distance of a decision of bundle_adjust()'s run from its threshold: accept / reject (|trial - kept| /
    kept), the stop tests (|ratio - 1|) and the depths' signs (|depth|)."""
    worst = res["depth"]
    for s in res["trace"]:
        if np.isfinite(s["trial"]):
            worst = min(worst, abs(s["trial"] - s["kept"]) / s["kept"])
        if np.isfinite(s["stop"]):
            worst = min(worst, abs(s["stop"] - 1.0))
    return float(worst)


TERM_OPS = 200            # rounded operations behind one term of S or g: the residual (30), J_x and J_p (60), the blocks and T W^T (110)
INV3_OPS = 3 * 3 * 3 * 4  # those of the three 3 x 3 Cholesky solves behind V^-1


def abs_sums(R, t, k0, k1, X, m, on, s2, lam):
    """(|S| (6, 6), |g| (6), the largest cond_2 of a row's damped V): the sums over the used rows of the absolute forms of sweep A's
    terms, |U_jk| + sum_c |T_jc| |W_kc| and |gp_j| + sum_c |T_jc| |gx_c| - what a term's rounding errors are relative to."""
    with np.errstate(all="ignore"):
        q = residual(R, t, k0, k1, X[on], m[on], s2)
        bl = blocks(R, k0, k1, X[on], q, lam)
        Vi, ok = inverse(bl["V"])
        T, W = np.abs(times_inverse(bl["W"], Vi)), np.abs(bl["W"])
        S, at = np.zeros((6, 6)), 0
        for j in range(6):
            for k in range(j, 6):
                S[j, k] = S[k, j] = (np.abs(bl["U"][:, at]) + (T[:, j] * W[:, k]).sum(axis=1))[ok].sum()
                at += 1
        g = np.array([(np.abs(bl["gp"][:, j]) + (T[:, j] * np.abs(bl["gx"])).sum(axis=1))[ok].sum() for j in range(6)])
        sv = np.linalg.svd(bl["V"][ok], compute_uv=False)
    return S, g, float((sv[:, 0] / sv[:, -1]).max())


def step_bound(step, k0, k1, m, on, s2):
    """What the reduced step of ONE solve may differ by between two float64 evaluations of the rule, in the manner of
    matches_ref.refine_step_bound: a term of S or g is TERM_OPS rounded operations and a 3 x 3 inverse whose relative error is
    INV3_OPS E cond(V), all relative to the term's absolute form (abs_sums); the sum is rounds + 8 + 4 additions deep; the damping
    and the gauge scale S by less than 1.5 + lambda; the 6 x 6 Cholesky adds CHOL_OPS E cond(A) |delta|.
    -> (bound on |delta - delta_ref|_2, cond_2(A), the largest cond_2(V))."""
    absS, absg, cond_v = abs_sums(step["R"], step["t"], k0, k1, step["X"], m, on, s2, step["lam"])
    rounds = -(-len(m) // mr.NT)
    rel = (TERM_OPS + INV3_OPS * cond_v + rounds + 8 + 4) * E
    sv = np.linalg.svd(step["A"], compute_uv=False)
    cond, inv = sv[0] / sv[-1], 1.0 / sv[-1]
    nd = np.sqrt((step["delta"] ** 2).sum())
    dA = rel * np.sqrt((absS * absS).sum()) * (1.5 + step["lam"])
    dg = rel * np.sqrt((absg * absg).sum())
    return inv * (dA * nd + dg) + mr.CHOL_OPS * E * cond * nd, cond, cond_v


OUT64 = ("pose64", "xyz64", "geom64", "cov_x64", "cov", "stats")
STORED32 = {"pose64": "pose", "xyz64": "xyz", "geom64": "geom", "cov_x64": "cov_x"}


def output_bounds(args, kwargs, res, h=1e-7):
    """What every float64 output of bundle_adjust(*args, **kwargs) = res may differ by between two float64 evaluations of the rule,
    element by element -> dict over OUT64 (the fp32 stores' half ulp not included), and the list of (step bound, cond(A), the largest
    cond(V)) per solve.  Two parts.  THE STEPS: solve k's reduced step differs by at most d_k = step_bound in every coordinate; to
    first order an output y then differs by at most sum_k sum_j |dy / d delta_kj| d_k, the derivatives taken here by one-sided
    differences of size h through the rule itself (perturb=), doubled for their own error; the accept sequence must not change
    under them.  THE LAST STAGE's own rounding: a sum of n terms is (TERM_OPS + INV3_OPS cond(V) + rounds + 12) E of its absolute
    form; C = (S0 + p u u^T)^-1 - u u^T / p differs by |C|^2 |dS0| + CHOL_OPS E cond |C| + 4 E / p; a point's covariance by
    |T|^2 dC plus the same relative error of |Vi| + |T|^2 |C|; the rotation moved by POSE_OPS E of an entry of R."""
    k0, k1, m, s2, on, R, t, len0 = (res[k] for k in ("k0", "k1", "m", "s2", "on", "R", "t", "len0"))
    n = len(m)
    on = on[:n]
    bounds = {k: np.zeros_like(res[k]) for k in OUT64}
    steps = []
    seq = [s["accepted"] for s in res["trace"]]
    for k, step in enumerate(res["trace"]):
        d, cond, cond_v = step_bound(step, k0, k1, m, on, s2)
        steps.append((d, cond, cond_v))
        for j in range(6):
            v = np.zeros(6)
            v[j] = h
            alt = bundle_adjust(*args, **kwargs, perturb=(k, v))
            assert [s["accepted"] for s in alt["trace"]] == seq, "the perturbation changed the accept sequence"
            for key in OUT64:
                with np.errstate(invalid="ignore"):
                    bounds[key] += 2.0 * np.abs(alt[key] - res[key]) / h * d
    # the last stage
    X = res["X"][:n]
    absS, _, cond_v = abs_sums(R, t, k0, k1, X, m, on, s2, 0.0)
    rounds = -(-n // mr.NT)
    rel = (TERM_OPS + INV3_OPS * cond_v + rounds + 12) * E
    A, _, _, pin = reduced(res["sums"], t, None)
    sv = np.linalg.svd(A, compute_uv=False)
    cond, norm_c = sv[0] / sv[-1], 1.0 / sv[-1] + 1.0 / pin
    dC = norm_c * norm_c * rel * np.sqrt((absS * absS).sum()) * 1.5 + mr.CHOL_OPS * E * cond * norm_c + 4.0 * E / pin
    bounds["cov"] += dC
    with np.errstate(all="ignore"):
        q = residual(R, t, k0, k1, X[on], m[on], s2)
        bl = blocks(R, k0, k1, X[on], q, 0.0)
        Vi, _ = inverse(bl["V"])
        T = times_inverse(bl["W"], Vi)
        t2 = (T * T).sum(axis=(1, 2))
        row = t2 * dC + rel * (np.sqrt((Vi * Vi).sum(axis=(1, 2))) + t2 * norm_c)
    rows_on = np.flatnonzero(res["on"])
    bounds["cov_x64"][rows_on] += (len0 * len0) * row[:, None]
    for key in ("pose64", "xyz64", "geom64"):
        with np.errstate(invalid="ignore"):
            bounds[key] += mr.POSE_OPS * E * np.abs(res[key])
    st, own = res["stats"], np.zeros(12)
    own[[1, 2]] = rel * np.abs(st[[1, 2]])
    own[7] = (rel + 4 * E) * st[7]
    with np.errstate(invalid="ignore"):
        C = res["cov"]
        own[8] = st[8] * (rel + 8 * E + 0.5 * 3 * dC / ((C[0, 0] + C[1, 1]) + C[2, 2]))
        own[9] = st[9] * (rel + 8 * E + 0.5 * 3 * dC / ((C[3, 3] + C[4, 4]) + C[5, 5]))
    own[10] = 16 * E * st[10] + mr.POSE_OPS * E * DEG
    bounds["stats"] += own
    return bounds, steps


# -------------------------------------------------------------------------------------------------------------- the fixtures
def triangulated(xy, count, K, pose):
    """(xyz fp32, flag) of tests/triangulate_ref.py's triangulate under pose."""
    tri = tr.triangulate(xy, count, K, pose)
    return tri["xyz"], tri["flag"]


GPU_ITERS = 10
GPU_SCALE = 2.0
GPU_FTOL = 1e-6           # at the default 1e-12 the last accepted gain of pair 0 is 3e-14 of the cost: round-off would decide the bytes


@functools.lru_cache(maxsize=None)
def gpu_case():
    """B = 6, N = 768 for cpn_bundle_adjust (seeds: matches_ref.refine_scene's 16 for every pair):
      0  600 rows of the noisy scene with outliers (0.5 px, 30 %), from refine_pose's result (10 passes, scale 2): some flags non-zero
      1  257 rows of the noisy scene without outliers from a start 8 degrees off in rotation and 17 in the direction of t: two
         rejected steps among eight accepted ones (from the scene's own 5 / 17 degree start every step is accepted)
      2  7 rows (below min_rows = 8): status 2
      3  0 rows: status 2
      4  300 rows under a pose with t = 0: status 2
      5  pair 0's rows with an inlier mask that drops every third row
    -> (xy (B, N, 4) fp32, counts, intrinsics (B, 2, 4, 4), poses (B, 4, 4) fp32, xyz (B, N, 3) fp32, flag (B, N) uint8, inlier (B, N) uint8)."""
    N = 768
    noisy = mr.refine_scene(n=1000, seed=16, noise_px=0.5, outliers=0.3)
    clean = mr.refine_scene(n=1000, seed=16, noise_px=0.5)
    refined = mr.refine_pose(noisy["xy"], 1000, noisy["intrinsics"], noisy["rel_pose"], 10, 2.0)[0].astype(np.float32)
    far = np.eye(4)
    far[:3, :3] = mr.rodrigues((1.0, -0.5, 0.7), 8.0) @ clean["R_true"]
    far[:3, 3] = clean["rel_pose"][:3, 3]
    still = refined.copy()
    still[:3, 3] = 0.0
    spec = [(noisy, 600, refined), (clean, 257, far.astype(np.float32)), (noisy, 7, refined), (noisy, 0, refined), (noisy, 300, still),
            (noisy, 600, refined)]
    xys, Ks, poses, pts, flags = [], [], [], [], []
    for sc, c, P in spec:
        xy = sc["xy"][:N].copy()
        xy[c:] = np.nan
        xyz, flag = triangulated(xy, c, sc["intrinsics"], P)
        xys.append(xy), Ks.append(sc["intrinsics"]), poses.append(np.asarray(P, dtype=np.float32)), pts.append(xyz), flags.append(flag)
    inlier = np.ones((len(spec), N), dtype=np.uint8)
    inlier[5, ::3] = 0
    return (np.stack(xys), np.asarray([c for _, c, _ in spec], dtype=np.int32), np.stack(Ks), np.stack(poses), np.stack(pts), np.stack(flags),
            inlier)


@functools.lru_cache(maxsize=None)
def gpu_args(b):
    """(args, kwargs) of bundle_adjust for pair b of gpu_case(), but iters."""
    xy, counts, K, poses, xyz, flag, inlier = gpu_case()
    return (xy[b], counts[b], K[b], poses[b], xyz[b], flag[b], inlier[b] if b == 5 else None), {"scale_px": GPU_SCALE, "ftol": GPU_FTOL}


@functools.lru_cache(maxsize=None)
def want_bounds(iters, b):
    """output_bounds of pair b of want(iters).  Shared."""
    args, kwargs = gpu_args(b)
    return output_bounds(args, dict(kwargs, iters=iters), want(iters)[b])


@functools.lru_cache(maxsize=None)
def want(iters=GPU_ITERS):
    """bundle_adjust() of every pair of gpu_case() at scale_px = GPU_SCALE and ftol = GPU_FTOL; pair 5 alone takes its inlier mask.
    Shared."""
    xy, counts, K, poses, xyz, flag, inlier = gpu_case()
    return [bundle_adjust(xy[b], counts[b], K[b], poses[b], xyz[b], flag[b], inlier[b] if b == 5 else None, iters=iters, scale_px=GPU_SCALE, ftol=GPU_FTOL)
            for b in range(len(xy))]
