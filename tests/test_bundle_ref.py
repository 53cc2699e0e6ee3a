"""tests/bundle_ref.py - the numpy restatement of cpn_bundle_adjust (round 27) - pinned on the CPU against forms it shares no code
with: central differences of the residual, the full (6 + 3 n)-square normal equations, a dense gauge-constrained inverse, round 26's
optimal triangulation, the scene's truth and a Monte-Carlo.  Bounds come from operation counts, condition numbers measured here
(and printed) and first-order perturbation; none from what the code gives.
"""
import numpy as np
import pytest

from tests import bundle_ref as br
from tests import matches_ref as mr
from tests import triangulate_ref as tr

E = br.E
NOISY = dict(n=1000, seed=16, noise_px=0.5, outliers=0.3)


def _truth(sc):
    P = np.eye(4)
    P[:3, :3], P[:3, 3] = sc["R_true"], sc["t_true"]
    return P


def _run(sc, pose, count, **kw):
    """bundle_adjust of the first `count` rows of a scene from `pose`, the points triangulated under it."""
    xy = sc["xy"][:count]
    pose = np.asarray(pose, dtype=np.float32)
    xyz, flag = br.triangulated(xy, count, sc["intrinsics"], pose)
    return br.bundle_adjust(xy, count, sc["intrinsics"], pose, xyz, flag, **kw), (xy, count, sc["intrinsics"], pose, xyz, flag)


def _small():
    """40 rows of the noisy scene without outliers at the scene's far start: the fixture of the dense comparisons."""
    sc = mr.refine_scene(n=1000, seed=16, noise_px=0.5)
    st = br.start(sc["xy"][:40], 40, sc["intrinsics"], sc["rel_pose"], *br.triangulated(sc["xy"][:40], 40, sc["intrinsics"], sc["rel_pose"]), None, 4.0)
    assert st["on"].sum() >= 36
    return sc, st


def _plain_residual(R, t, K, X, m):
    """The 4 pixel residuals in matrix form (no shared code with bundle_ref.residual)."""
    Y = (X - t) @ R
    f0, c0, f1, c1 = np.array([K[0][0, 0], K[0][1, 1]]), K[0][:2, 2], np.array([K[1][0, 0], K[1][1, 1]]), K[1][:2, 2]
    return np.concatenate((f0 * X[:, :2] / X[:, 2:] + c0 - m[:, :2], f1 * Y[:, :2] / Y[:, 2:] + c1 - m[:, 2:]), 1)


def _moved(R, t, X, dp, dX):
    """The rule's update of the whole state: R <- exp([om]x) R, t <- (t + dt) / len, X <- (X + dX) / len."""
    tn = t + dp[3:]
    ln = np.linalg.norm(tn)
    th = np.linalg.norm(dp[:3])
    Q = mr.rodrigues(dp[:3] / th, np.degrees(th)) if th > 0 else np.eye(3)
    return Q @ R, tn / ln, (X + dX) / ln


def test_jacobians_against_central_differences():
    """J_p and J_x against central differences (h = 1e-6) of the residual THROUGH the rule's update - the left rotation step, the
    renormalised t and the points divided by the same length.  Truncation h^2 |f'''| / 6 and rounding E |f| / h are both below
    1e-7 of an entry's scale (|J| up to 600 px per unit); the bound is 1e-6 (1 + |J|)."""
    sc, st = _small()
    R, t, X, m, on = st["R"], st["t"], st["X"][st["on"]], st["m"][st["on"]], st["on"]
    K = sc["intrinsics"].astype(np.float64)
    q = br.residual(R, t, st["k0"], st["k1"], X, m, 4.0)
    Jx, Jp = br.jacobians(R, st["k0"], st["k1"], X, q)
    assert np.abs(np.stack(q["r"], 1) - _plain_residual(R, t, K, X, m)).max() < 1e-10
    h, zero = 1e-6, np.zeros_like(X)

    def at(d):
        Rn, tn, Xn = _moved(R, t, X, d, zero)
        return _plain_residual(Rn, tn, K, Xn, m)

    for j in range(6):
        d = np.zeros(6)
        d[j] = h
        fd = (at(d) - at(-d)) / (2 * h)
        want = np.stack([np.zeros(len(X)), np.zeros(len(X)), Jp[0][j], Jp[1][j]], 1)
        assert (np.abs(fd - want) <= 1e-6 * (1 + np.abs(want))).all(), (j, np.abs(fd - want).max())
    for c in range(3):
        dX = np.zeros_like(X)
        dX[:, c] = h
        fd = (_plain_residual(R, t, K, X + dX, m) - _plain_residual(R, t, K, X - dX, m)) / (2 * h)
        want = np.stack([Jx[a][c] for a in range(4)], 1)
        assert (np.abs(fd - want) <= 1e-6 * (1 + np.abs(want))).all(), (c, np.abs(fd - want).max())


def _full_system(st, s2, lam):
    """(H (6 + 3 n square, undamped), b, the blocks) of the used rows, dense, from the Jacobians alone."""
    R, t, on = st["R"], st["t"], st["on"]
    X, m = st["X"][on], st["m"][on]
    q = br.residual(R, t, st["k0"], st["k1"], X, m, s2)
    Jx, Jp = br.jacobians(R, st["k0"], st["k1"], X, q)
    n = len(X)
    J = np.zeros((4 * n, 6 + 3 * n))
    r = np.stack(q["r"], 1).reshape(-1)
    for i in range(n):
        for a in range(2):
            J[4 * i + 2 + a, :6] = [Jp[a][j][i] for j in range(6)]
        for a in range(4):
            J[4 * i + a, 6 + 3 * i:9 + 3 * i] = [Jx[a][c][i] for c in range(3)]
    w = np.repeat(q["w"], 4)
    return J.T @ (w[:, None] * J), J.T @ (w * r), n


def _schur_step(st, s2, lam, defect=None):
    on = st["on"]
    sums = br.sweep_a(st["R"], st["t"], st["k0"], st["k1"], st["X"], st["m"], on, s2, lam)
    A, g, S, pin = br.reduced(sums, st["t"], lam)
    delta = mr.solve6(A, g)
    dX = br.back_substitute(st["R"], st["t"], st["k0"], st["k1"], st["X"][on], st["m"][on], s2, lam, delta, defect)
    return delta, dX, S, pin


def _schur_gap(defect=None, lam=1e-3):
    """(the largest |difference| of (dp, dX) between the restatement's Schur step and the dense solve, relative to the step; the
    tolerance cond(H) E 8: pose radians against points, a cond near 1e8)."""
    sc, st = _small()
    delta, dX, S, pin = _schur_step(st, 4.0, lam, defect)
    H, b, n = _full_system(st, 4.0, lam)
    Hd = H.copy()
    for i in range(6, 6 + 3 * n):
        Hd[i, i] += lam * H[i, i]
    for j in range(6):
        Hd[j, j] += lam * S[j, j]                                        # the rule damps the REDUCED diagonal
    Hd[3:6, 3:6] += pin * np.outer(st["t"], st["t"])
    full = np.linalg.solve(Hd, -b)
    mine = np.concatenate((delta, dX.reshape(-1)))
    return float(np.abs(full - mine).max() / np.abs(full).max()), float(np.linalg.cond(Hd) * E * 8)


def test_schur_step_against_the_full_normal_equations():
    """(dp, dX) of the restatement against np.linalg.solve of the full damped, gauge-pinned system of 40 rows (6 + 3 n = about
    120 unknowns); tolerance 8 cond(H) E, printed."""
    gap, tol = _schur_gap()
    print(f"Schur step against the dense solve: relative gap {gap:.3g}, tolerance {tol:.3g}")
    assert gap <= tol < 1e-6


def test_hard_properties():
    """The kept cost never rises; iters = 0 changes nothing (the pose and the used points in their fp32 bits); with lambda = 0
    |S u| / |S| for u = (0, t) is at round-off (below cond(V) E 1e3) and grows in proportion to lambda; the output pose has
    |t| = len0 and R^T R = the input's R^T R - I for an orthonormal input: the rule steps on the left by exact rotations and never
    re-orthonormalises, so an fp32 input's 6e-8 stays, as it does in refine_pose."""
    sc = mr.refine_scene(**NOISY)
    for res in br.want(10):
        costs = [s["kept"] for s in res["trace"]] + ([res["stats"][1]] if res["trace"] else [])
        assert all(b <= a for a, b in zip(costs, costs[1:]))
    res, args = _run(sc, sc["rel_pose"], 300, iters=0, scale_px=2.0)
    on = res["on"]
    assert res["pose"].tobytes() == args[3].tobytes() and res["xyz"][on].tobytes() == args[4][on].tobytes() and on.sum() > 150
    assert res["stats"][0] == res["stats"][1] and res["stats"][4] == res["stats"][5] == 0 and res["stats"][10] == 0
    _, st = _small()
    ratios = []
    for lam in (0.0, 1e-6, 1e-5):
        S = br.reduced(br.sweep_a(st["R"], st["t"], st["k0"], st["k1"], st["X"], st["m"], st["on"], 4.0, lam), st["t"], None)[2]
        ratios.append(np.linalg.norm(S @ np.concatenate((np.zeros(3), st["t"]))) / np.linalg.norm(S))
    cond_v = br.abs_sums(st["R"], st["t"], st["k0"], st["k1"], st["X"], st["m"], st["on"], 4.0, 0.0)[2]
    print(f"|S u| / |S| at lambda 0, 1e-6, 1e-5: {ratios}; largest cond(V) {cond_v:.3g}")
    assert ratios[0] <= cond_v * E * 1e3 and 9 < ratios[2] / ratios[1] < 11 and ratios[1] > 1e-9
    poses = br.gpu_case()[3].astype(np.float64)
    for b, res in enumerate(br.want(10)):
        if res["stats"][11] == 0:                                        # a left step keeps R^T R: the output's is the input's
            P, R0 = res["pose64"], poses[b][:3, :3]
            assert np.abs(P[:3, :3].T @ P[:3, :3] - R0.T @ R0).max() < 64 * E * (1 + len(res["trace"]))
            assert abs(np.linalg.norm(P[:3, 3]) / res["len0"] - 1) < 8 * E
    res = _round26_gap(0.5)[2]                                           # and from an orthonormal float64 pose it is I
    assert np.abs(res["R"].T @ res["R"] - np.eye(3)).max() < 64 * E * (1 + len(res["trace"]))


def _round26_gap(noise, defect=None):
    """From a float64, orthonormal start (pose64: the comparison is made in float64; an fp32 pose's R^T R - I of 5e-8 alone moves
    the points by 6e-7 of |X|, which is what the prototype's 3e-7 was).  At the converged state, per used inlier: |X_ba - X_round26| / |X| under the same float64 pose, and the bound: twice the
    point's own Newton decrement |Vi gx| (what the last LM step left undone, to first order) over |X|, plus 1e-12 for round 26's
    three passes (within 1e-15 px of convergence on a match within 2 px) and the rounding of both."""
    sc = mr.refine_scene(n=300, seed=16, noise_px=noise)
    Pt = _truth(sc)
    Pt[:3, :3] = mr.rodrigues((1.0, -0.5, 0.7), 0.5) @ Pt[:3, :3]       # half a degree off, orthonormal in float64
    xyz, _, flag = tr.rows64(sc["xy"].astype(np.float64), sc["intrinsics"].astype(np.float64), Pt)[:3]
    res = br.bundle_adjust(sc["xy"], 300, sc["intrinsics"], Pt, xyz.astype(np.float32), flag, iters=40, scale_px=2.0, ftol=0.0, defect=defect,
                           pose64=Pt)
    on = np.flatnonzero(res["on"] & (res["geom64"][:, 2] < 2.0))
    P, K = res["pose64"], sc["intrinsics"].astype(np.float64)
    X26 = tr.rows64(res["m"][on], K, P)[0]
    undone = np.linalg.norm(tr.rows64(res["m"][on], K, P, passes=tr.PASSES + 1)[0] - X26, axis=1)      # what a fourth pass would move
    Xba = res["xyz64"][on]
    q = br.residual(res["R"], res["t"], res["k0"], res["k1"], res["X"][on], res["m"][on], 4.0)
    bl = br.blocks(res["R"], res["k0"], res["k1"], res["X"][on], q, 0.0)
    Vi, _ = br.inverse(bl["V"])
    dec = np.linalg.norm(np.einsum("nab,nb->na", Vi, bl["gx"]), axis=1) * res["len0"]
    norm = np.linalg.norm(Xba, axis=1)
    return np.linalg.norm(Xba - X26, axis=1) / norm, 2.0 * (dec + undone) / norm + 1e-12, res


@pytest.mark.parametrize("noise", [0.0, 0.5])
def test_points_against_round_26(noise):
    """At the converged pose every used inlier's point is round 26's optimal triangulation under that same float64 pose: both
    minimise the same squared reprojection distance of the row."""
    gap, bound, res = _round26_gap(noise)
    print(f"noise {noise}: {len(gap)} rows, largest gap {gap.max():.3g} of |X|, largest gap / bound {(gap / bound).max():.3g}; "
          f"accepted {int(res['stats'][4])}, rejected {int(res['stats'][5])}")
    assert len(gap) > 250 and (gap <= bound).all()


def test_recovery_on_exact_matches():
    """Exact matches (the coordinates rounded to fp32), a start 1 degree off with the points triangulated under it: the pose
    returns to the truth within 1.5 times the first-order effect of the coordinates' rounding, sum_i,a |(C Jr_i^T)_ja|
    ulp32(x_ia) / 2 with Jr_i = J_p - J_x Vi W^T the row's reduced Jacobian (test_triangulate_ref.py's form of bound), per
    coordinate of (om, dt)."""
    sc = mr.refine_scene()
    Pt = _truth(sc)
    P = Pt.copy()
    P[:3, :3] = mr.rodrigues((0.2, -1.0, 0.4), 1.0) @ Pt[:3, :3]
    res, _ = _run(sc, P, 400, iters=30, scale_px=2.0, ftol=0.0)
    assert res["stats"][11] == 0 and res["stats"][3] > 390
    on = res["on"]
    R, t, X, m = res["R"], res["t"], res["X"][on], res["m"][on]
    q = br.residual(R, t, res["k0"], res["k1"], X, m, 4.0)
    bl = br.blocks(R, res["k0"], res["k1"], X, q, 0.0)
    Vi, _ = br.inverse(bl["V"])
    Jx = np.stack([np.stack(row, 1) for row in bl["Jx"]], 1)                      # (n, 4, 3)
    Jp = np.zeros((len(X), 4, 6))
    Jp[:, 2:] = np.stack([np.stack(row, 1) for row in bl["Jp"]], 1)
    Jr = Jp - np.einsum("nac,ncd,njd->naj", Jx, Vi, bl["W"])
    CJ = np.abs(np.einsum("jk,nak->naj", res["cov"], Jr * q["w"][:, None, None]))
    bound = np.einsum("naj,na->j", CJ, mr.half_ulp32(m))
    dR = R @ sc["R_true"].T
    om = np.array([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]]) / 2.0
    tt = sc["t_true"] / np.linalg.norm(sc["t_true"])
    err = np.abs(np.concatenate((om, t - tt)))
    print("recovery on exact matches: |error| of (om, dt)", err, "; 1.5 bound", 1.5 * bound, "; degrees", mr.pose_errors(res["pose64"], sc))
    assert (err <= 1.5 * bound + 1e-12).all()


def test_convergence_from_the_far_start():
    """From the scene's 5 / 17 degree start (n = 200, 0.5 px noise): the pose ends within 4 predicted standard deviations of the
    truth - stats[8] and stats[9], sigma sqrt(tr C) in degrees - and the cost falls by more than 10 times.  The scene's noise is on
    view 1 alone, half of the coordinates: sigma-hat is near 0.5 / sqrt(2) = 0.35 (within a quarter of it; the robust weight lowers it)."""
    sc = mr.refine_scene(n=200, seed=16, noise_px=0.5)
    res, _ = _run(sc, sc["rel_pose"], 200, iters=30, scale_px=2.0)
    rot, tra = mr.pose_errors(res["pose64"], sc)
    st = res["stats"]
    print(f"far start: {rot:.3f}, {tra:.3f} degrees from the truth after {int(st[4])} accepted and {int(st[5])} rejected steps; predicted "
          f"{st[8]:.3f}, {st[9]:.3f}; sigma {st[7]:.3f}")
    assert st[11] == 0 and rot <= 4 * st[8] and tra <= 4 * st[9] and st[1] < st[0] / 10 and 0.26 < st[7] < 0.45


def _dense_covariance(st, s2):
    """(the pose block, the points' blocks) of N (N^T H N)^-1 N^T: H the full undamped normal matrix, N an orthonormal basis of
    the complement of (0, t, 0, ..)."""
    H, _, n = _full_system(st, s2, 0.0)
    u = np.zeros(6 + 3 * n)
    u[3:6] = st["t"]
    Q = np.linalg.svd(np.eye(len(u)) - np.outer(u, u))[0][:, :-1]
    full = Q @ np.linalg.inv(Q.T @ H @ Q) @ Q.T
    return full[:6, :6], np.stack([full[6 + 3 * i:9 + 3 * i, 6 + 3 * i:9 + 3 * i] for i in range(n)]), np.linalg.cond(Q.T @ H @ Q)


def _covariance_gap(defect=None):
    _, st = _small()
    on = st["on"]
    sums = br.sweep_a(st["R"], st["t"], st["k0"], st["k1"], st["X"], st["m"], on, 4.0, 0.0)
    C = br.covariance(sums, st["t"], defect)
    Cov, _ = br.point_covariances(st["R"], st["t"], st["k0"], st["k1"], st["X"][on], st["m"][on], 4.0, C)
    Cd, Xd, cond = _dense_covariance(st, 4.0)
    tri = np.stack([Xd[:, a, c] for a in range(3) for c in range(a, 3)], 1)
    return float(max(np.abs(C - Cd).max() / np.abs(Cd).max(), (np.abs(Cov - tri) / np.abs(tri).max(axis=1, keepdims=True)).max())), float(cond * E * 8)


def test_covariances_against_the_dense_inverse():
    """cov and cov_x are the pose and the point blocks of N (N^T H N)^-1 N^T; tolerance 8 cond(N^T H N) E, printed."""
    gap, tol = _covariance_gap()
    print(f"covariances against the dense gauge-constrained inverse: relative gap {gap:.3g}, tolerance {tol:.3g}")
    assert gap <= tol < 1e-6


def test_covariance_monte_carlo():
    """120 noise draws (sigma = 0.5 px on all four coordinates of 80 exact rows, scale_px = 1e6: no robust weight) from the truth:
    the empirical second moments of the rotation and translation errors over sigma^2 tr C, each with its sampling standard
    deviation sqrt(2 sum l^2 / (M (sum l)^2)) (l the block's predicted eigenvalues); asserted within 4 of them; sigma-hat's mean
    within 4 standard errors of 0.5 (its own standard deviation is sigma / sqrt(2 dof))."""
    sc = mr.refine_scene(n=80, seed=16)
    Pt, K = _truth(sc), sc["intrinsics"]
    rng = np.random.default_rng(27)
    xyz0, _ = br.triangulated(sc["xy"], 80, K, Pt.astype(np.float32))
    clean = br.bundle_adjust(sc["xy"], 80, K, Pt.astype(np.float32), xyz0, np.zeros(80, dtype=np.uint8), iters=10, scale_px=1e6)
    C, M, sigma = clean["cov"], 120, 0.5
    tt = sc["t_true"] / np.linalg.norm(sc["t_true"])
    errs, sig = [], []
    for _ in range(M):
        xy = (sc["xy"].astype(np.float64) + rng.normal(scale=sigma, size=(80, 4))).astype(np.float32)
        xyz, flag = br.triangulated(xy, 80, K, Pt.astype(np.float32))
        res = br.bundle_adjust(xy, 80, K, Pt.astype(np.float32), xyz, flag, iters=10, scale_px=1e6)
        assert res["stats"][11] == 0 and res["stats"][3] == 80
        dR = res["R"] @ sc["R_true"].T
        errs.append(np.concatenate((np.array([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]]) / 2.0, res["t"] - tt)))
        sig.append(res["stats"][7])
    errs = np.array(errs)
    for name, sl in (("rotation", slice(0, 3)), ("translation", slice(3, 6))):
        lam = np.linalg.eigvalsh(C[sl, sl])
        ratio = (errs[:, sl] ** 2).sum(axis=1).mean() / (sigma ** 2 * lam.sum())
        sd = np.sqrt(2.0 * (lam ** 2).sum() / (M * lam.sum() ** 2))
        print(f"Monte-Carlo, {name}: empirical / predicted variance {ratio:.3f} +- {sd:.3f}")
        assert abs(ratio - 1.0) <= 4.0 * sd
    dof = 4 * 80 - 3 * 80 - 5
    print(f"Monte-Carlo, sigma-hat: mean {np.mean(sig):.4f} (truth {sigma}), standard error {sigma / np.sqrt(2 * dof * M):.4f}; rows - 5 = 75 "
          f"is the formula's divisor, the degrees of freedom are {dof}")
    assert abs(np.mean(sig) - sigma * np.sqrt(dof / 75.0)) <= 4.0 * sigma * np.sqrt(dof / 75.0) / np.sqrt(2 * dof * M) + 0.01


def test_margins_of_the_gpu_fixtures():
    """What licenses the exact comparisons on the GPU: over gpu_case() (refine_scene's seed 16) at iters 0, 1 and 10 no accept /
    reject comparison, no stop test and no depth sign is within 1e-9 of its threshold; pair 1 has steps of both kinds."""
    for iters in (0, 1, 10):
        for b, res in enumerate(br.want(iters)):
            if res["stats"][11] != 2:
                margin = br.margins(res)
                print(f"iters {iters} pair {b}: margin {margin:.3g}, sequence {''.join('A' if s['accepted'] else 'R' for s in res['trace'])}")
                assert margin >= br.MARGIN
    st = br.want(10)[1]["stats"]
    assert st[4] >= 1 and st[5] >= 1
    assert [int(r["stats"][11]) for r in br.want(10)] == [0, 0, 2, 2, 2, 0] and [int(r["stats"][3]) for r in br.want(10)] == [473, 257, 6, 0, 0, 320]
    flags = br.gpu_case()[5][0][:600]
    assert (flags != 0).any() and (flags == 0).sum() > 400


def _scale_check(defect=None):
    """The trial cost of the first step from the far start equals the cost of the SAME step without any renormalisation - (R',
    t + dt, X + dX), which the residual cannot tell from the rule's (R', t', (X + dX) / len) - in matrix form."""
    sc, st = _small()
    on = st["on"]
    delta, dX, _, _ = _schur_step(st, 4.0, 1e-3)
    tn = st["t"] + delta[3:]
    ln = np.linalg.norm(tn)
    Rn, tu = mr.apply_step(st["R"], st["t"], delta)
    _, trial, _ = br.sweep_b(st["R"], st["t"], Rn, tu, ln, st["k0"], st["k1"], st["X"], st["m"], on, 4.0, 1e-3, delta, defect)
    r = _plain_residual(Rn, tn, sc["intrinsics"].astype(np.float64), st["X"][on] + dX, st["m"][on])
    e2 = (r * r).sum(axis=1)
    return abs(trial - ((e2 / 2) / (1 + e2 / 4.0)).sum()) / trial


def _lambda_check(defect=None):
    """Every rejection multiplies the next solve's lambda by 4, every accepted step divides it by 3."""
    args, kw = br.gpu_args(1)
    trace = br.bundle_adjust(*args, **kw, iters=10, defect=defect)["trace"]
    assert any(not s["accepted"] for s in trace[:-1])
    return all(b["lam"] == (a["lam"] / 3.0 if a["accepted"] else 4.0 * a["lam"]) for a, b in zip(trace, trace[1:]))


def test_seeded_defects_are_caught():
    """Each of bundle_ref.DEFECTS fails the check that is there for it, and the rule passes it.  (The rule takes no derivative of
    the weight, so there is none to freeze.)"""
    assert _scale_check() < 1e-12 and _scale_check("no len") > 1e-3
    assert _lambda_check() and not _lambda_check("stale lambda")
    gap, tol = _schur_gap()
    bad, _ = _schur_gap("backsub sign")
    assert gap <= tol and bad > 1e-3
    gap, tol = _covariance_gap()
    bad, _ = _covariance_gap("no gauge")
    assert gap <= tol and bad > 1e-3
    assert set(br.DEFECTS) == {"no len", "stale lambda", "backsub sign", "no gauge"}
