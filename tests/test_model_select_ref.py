"""tests/model_select_ref.py, the restatement of cpn_refine_homography and cpn_model_gric (include/coponerf_hip.h, round 23), held
to independent forms on the CPU: the Jacobians to finite differences, the residual to its meaning as a distance, the refinement to
the truth of exact scenes, the decisions to the scenes' names, and every seeded defect to at least one of these assertions.
"""
import numpy as np
import pytest

from tests import homography_ref as hr
from tests import matches_ref as mr
from tests import model_select_ref as ms
from tests import ransac5_ref as r5

E = ms.E
SIGMAS = (0.35, 0.5, 0.7, 1.0)
SEEDS = (0, 1, 2)
Y_OPS = 32                                                           # the depth of y (model_select_ref's docstring: 30)


def _norm_points(xy, K):
    """Normalised points in float64 WITHOUT the fp32 cast of the fixtures: the tests below displace matches by less than an ulp32."""
    k0, k1 = mr.cam_of(K[0]), mr.cam_of(K[1])
    return k0, k1, ((xy[:, 0] - k0[2]) / k0[0], (xy[:, 1] - k0[3]) / k0[1], (xy[:, 2] - k1[2]) / k1[0], (xy[:, 3] - k1[3]) / k1[1])


def _y(H, k0, k1, pts):
    s = ms.sampson_h(H, k0, k1, *pts)
    return np.stack((s["y0"], s["y1"])), s


def _hostile():
    """The wall's refined H and five matches, the first with m_2 = (H b)_2 = 1e-3: its view-1 point lies almost on the line that H
    sends to infinity."""
    sc, _, res = ms.scene_selection("wall")
    H = res["producers"]["plane_H"]
    xy = sc["xy"][:5].astype(np.float64).copy()
    k1 = mr.cam_of(sc["intrinsics"][1])
    b1 = (xy[0, 3] - k1[3]) / k1[1]
    b0 = (1e-3 - H[7] * b1 - H[8]) / H[6]
    xy[0, 2] = b0 * k1[0] + k1[2]
    return sc, H, xy


def _jacobian_errors(H, dirs, k0, k1, pts, defect=None, step=1e-6):
    """-> (|J - central difference|, the finite-difference error estimate), each (2, len(dirs), n).  The estimate: the difference of
    the central differences at `step` and 2 `step` (three times the truncation error of the former) plus the rounding of y itself,
    Y_OPS E times y's absolute form, in both evaluations, over 2 `step`."""
    y, s = _y(H, k0, k1, pts)
    mag = ms.sampson_h(np.abs(H), k0, k1, *(np.abs(p) for p in pts), true=s)
    ymag = np.stack((mag["y0"], mag["y1"]))
    errs, bounds = [], []
    for d in dirs:
        J = np.stack(ms.along(s, d, k0, k1, defect=defect))
        fd = [(_y(H + h * d, k0, k1, pts)[0] - _y(H - h * d, k0, k1, pts)[0]) / (2.0 * h) for h in (step, 2.0 * step)]
        errs.append(np.abs(J - fd[0]))
        bounds.append(np.abs(fd[0] - fd[1]) + Y_OPS * E * ymag * 2.0 / (2.0 * step) * 2.0)
    return np.stack(errs, 1), np.stack(bounds, 1)


@pytest.mark.parametrize("case", ("wall", "hostile"))
def test_jacobians_against_central_differences(case):
    """J_y = (dy0, dy1) along every direction of both modes against central differences of y at the wall's refined H: on the wall's
    first 50 matches, and on five matches of which one has m_2 = 1e-3.  Bound: the finite-difference error estimate.  The frozen-
    whitening shortcut and a dropped dl11 term both miss it by orders of magnitude."""
    if case == "wall":
        sc, _, res = ms.scene_selection("wall")
        H, xy = res["producers"]["plane_H"], sc["xy"][:50].astype(np.float64)
    else:
        sc, H, xy = _hostile()
    k0, k1, pts = _norm_points(xy, sc["intrinsics"])
    Rn = ms.nearest_rotation(H)
    for mode, state, dirs in ((0, H, ms.unit_directions()), (1, Rn, ms.rotation_directions(Rn))):
        err, bound = _jacobian_errors(state, dirs, k0, k1, pts)
        print(case, "mode", mode, "largest error / bound", float((err / bound).max()), "largest bound", float(bound.max()),
              "largest |J|", float(max(np.abs(np.stack(ms.along(_y(state, k0, k1, pts)[1], d, k0, k1))).max() for d in dirs)))
        assert (err <= bound).all()
        for defect in ("dropped dl11", "frozen whitening"):
            bad, _ = _jacobian_errors(state, dirs, k0, k1, pts, defect=defect)
            assert (bad > 100.0 * bound).any(), (mode, defect)
    if case == "hostile":
        assert abs((H[6] * pts[2][0] + H[7] * pts[3][0]) + H[8] - 1e-3) < 1e-12


def test_the_residual_is_the_distance_to_the_model():
    """For matches that satisfy H exactly, displaced by delta pixels along random directions, e^2 / |P delta|^2 -> 1 with P the
    projector onto the row space of the constraint's Jacobian J in the pixels: e is, to first order, the distance in pixels from the
    match to the matches that satisfy H.  The constraint is bilinear in the two points, so the ratio departs from 1 at first order in
    delta over the focal length: held to 20 delta / f over three decades, and to shrink ten-fold (between 5 and 20) per decade."""
    sc = r5.wall_scene(**r5.WALL)
    H = ms.wall_truth()
    k0, k1 = mr.cam_of(sc["intrinsics"][0]), mr.cam_of(sc["intrinsics"][1])
    rng = np.random.default_rng(23)
    n = 200
    x1 = rng.uniform(0.0, 256.0, size=(n, 2))
    b0, b1 = (x1[:, 0] - k1[2]) / k1[0], (x1[:, 1] - k1[3]) / k1[1]
    m = [(H[3 * i] * b0 + H[3 * i + 1] * b1) + H[3 * i + 2] for i in range(3)]
    base = np.stack((k0[0] * m[0] / m[2] + k0[2], k0[1] * m[1] / m[2] + k0[3], x1[:, 0], x1[:, 1]), 1)      # exact matches, float64
    _, _, pts = _norm_points(base, sc["intrinsics"])
    s = ms.sampson_h(H, k0, k1, *pts)
    assert s["ok"].all() and s["e2"].max() < 1e-20
    J = np.zeros((n, 2, 4))
    J[:, 0, 0], J[:, 0, 2], J[:, 0, 3], J[:, 1, 1], J[:, 1, 2], J[:, 1, 3] = (s[k] for k in ("J00", "J02", "J03", "J11", "J12", "J13"))
    direction = rng.normal(size=(n, 4))
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    worst = []
    for delta in (1e-2, 1e-3, 1e-4):
        d = delta * direction
        _, _, moved = _norm_points(base + d, sc["intrinsics"])
        e2 = ms.sampson_h(H, k0, k1, *moved)["e2"]
        Pd2 = np.array([d[i] @ np.linalg.pinv(J[i]) @ J[i] @ d[i] for i in range(n)])
        worst.append(float(np.abs(e2 / Pd2 - 1.0).max()))
        print("delta", delta, "largest |e^2 / |P delta|^2 - 1|", worst[-1])
        assert worst[-1] <= 20.0 * delta / k0[0]
    assert 5.0 < worst[0] / worst[1] < 20.0 and 5.0 < worst[1] / worst[2] < 20.0


def _perturbed(truth, size, seed):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=9)
    return truth + size * d / np.linalg.norm(d)


def test_recovery_of_exact_scenes():
    """From the wall without noise or outliers and a start 1e-2 (Frobenius) off the true unit h, ten passes of mode 0 return to the
    truth; from the pure rotation without noise and a start turned by 1e-2 / sqrt(2) rad, ten passes of mode 1 return to the true R.
    What is left is the fp32 rounding of the coordinates: the tolerance is model_select_ref.rounding_tolerance, a first-order bound on
    it, not a figure from the run.  Without its gauge the plane's normal matrix is flat along h: h^T A h must reach tr / 9."""
    wall = r5.wall_scene(noise_px=0.0, outliers=0.0)
    truth = ms.wall_truth()
    start = _perturbed(truth, 1e-2, 1)
    H, pose, stats, trace = ms.refine_homography(wall["xy"], 1000, wall["intrinsics"], start, 0, 10, 2.0)
    tol = ms.rounding_tolerance(trace[-1], 0)
    d0, d1 = np.linalg.norm(start / np.linalg.norm(start) - truth), np.linalg.norm(H - truth)
    print("wall: start", d0, "reached", d1, "tolerance", tol, "reached / start", d1 / d0, "stats", stats)
    assert stats[7] == 0 and stats[6] == 10 and stats[3] == 1000 and d1 <= tol < 1e-3 * d0
    assert abs(np.linalg.norm(H) - 1.0) < 1e-15 and np.linalg.det(H.reshape(3, 3)) > 0 and np.array_equal(pose, np.eye(4))
    assert abs(stats[4] - np.linalg.norm(H - start / np.linalg.norm(start))) < 1e-12
    sv = np.linalg.svd(H.reshape(3, 3), compute_uv=False)
    assert abs(stats[5] - (sv[0] - sv[2]) / sv[1]) < 1e-12
    first = trace[0]
    h = first["H"]
    assert h @ first["A"] @ h >= np.trace(first["M"]) / 9.0
    bare = ms.damped(first["sums"], 9, h, defect="no gauge")[0]
    assert h @ bare @ h < np.trace(first["M"]) / 90.0               # the seeded defect: caught by the assertion above

    turn = hr.rotation_scene(noise_px=0.0, outliers=0.0)
    R_true = turn["R_true"]
    R_start = mr.rodrigues((0.4, -1.0, 0.3), np.degrees(1e-2 / np.sqrt(2.0))) @ R_true
    R, pose, stats, trace = ms.refine_homography(turn["xy"], 1000, turn["intrinsics"], R_start.reshape(9), 1, 10, 2.0)
    tol = ms.rounding_tolerance(trace[-1], 1)
    d0, d1 = np.linalg.norm(R_start - R_true), np.linalg.norm(R.reshape(3, 3) - R_true)
    print("rotation: start", d0, "reached", d1, "tolerance", tol, "reached / start", d1 / d0, "stats", stats)
    assert stats[7] == 0 and stats[6] == 10 and stats[5] == 0 and d1 <= tol < 1e-3 * d0
    assert abs(d0 - 1e-2) < 1e-6 and np.array_equal(pose[:3, :3], R.reshape(3, 3)) and not pose[:3, 3].any()
    assert abs(stats[4] - mr.rotation_angle_deg(R.reshape(3, 3), ms.nearest_rotation(R_start.reshape(9)).reshape(3, 3))) < 1e-9


@pytest.mark.parametrize("name", ("wall", "curved", "rotation"))
def test_the_cost_never_rises(name):
    """On the three noisy scenes, from homography_pose's winner at 256 hypotheses, the robust cost of every pass is at most the one
    before it, in both modes - up to the rounding of the cost's own sum once the passes have converged: a sum of non-negative terms,
    each at most RHO_OPS operations deep, added rounds + 8 deep, so two evaluations differ by at most (RHO_OPS + rounds + 8) E
    times the cost each."""
    sc, _, res = ms.scene_selection(name)
    for mode in (0, 1):
        _, _, stats, trace = ms.refine_homography(sc["xy"], 1000, sc["intrinsics"], res["producers"]["homography_H"], mode, 10, 2.0)
        NP = 9 if mode == 0 else 3
        cost = np.array([t["sums"][NP * (NP + 1) // 2 + NP] for t in trace])
        print(name, "mode", mode, "cost", cost)
        assert len(cost) == 11 and stats[0] == cost[0] and stats[1] == cost[-1] 
        assert (np.diff(cost) <= 2.0 * (ms.RHO_OPS + 4 + 8) * E * cost[:-1]).all()


def _decisions(defect=None):
    out = []
    for name, _ in hr.scenes():
        for seed in SEEDS:
            sc, rel, res = ms.scene_selection(name, 256, seed)
            pr = res["producers"]
            for sigma in SIGMAS:
                gric, label, stats, info = ms.model_gric(sc["xy"], 1000, sc["intrinsics"], pr["refined_pose"].astype(np.float32), pr["plane_H"],
                                                         pr["rotation_H"], pr["avail"], sigma, defect=defect)
                out.append((name, seed, sigma, gric, stats, info, ms.unrefined_pick(sc, rel, pr, sigma) if defect is None else None))
    return out


def test_the_decisions_and_their_margins():
    """homography_ref.scenes() x seeds 0, 1, 2 at 256 hypotheses x sigma_px in {0.35, 0.5, 0.7, 1.0}: after the refinement the wall
    picks the plane, the curved scene E and the pure rotation the rotation alone in all 36 cases, every time by at least 1000 times
    the summation bound, and no x = e^2 / sigma^2 lies within 1e-9 of its cap: no rounding of the GPU can flip a decision or a
    label.  Printed beside them, not asserted: what the UNREFINED winners would pick."""
    wrong_unrefined = 0
    for name, seed, sigma, gric, stats, info, (raw_pick, raw_gric) in _decisions():
        print(f"{name:8s} seed {seed} sigma {sigma}: gric (E, plane, rotation) {np.round(gric, 1)} pick {int(stats[0])} margin "
              f"{stats[5]:.1f} bound {info['bound'].max():.1e} cap margin {info['cap_margin']:.1e} | unrefined {np.round(raw_gric, 1)} "
              f"pick {raw_pick}")
        wrong_unrefined += raw_pick != ms.EXPECTED[name]
        assert info["in"] == [True, True, True] and stats[6] == 0
        assert int(stats[0]) == ms.EXPECTED[name], (name, seed, sigma, gric)
        assert stats[5] >= 1000.0 * info["bound"].max()
        assert info["cap_margin"] >= ms.CAP_MARGIN
    print("unrefined winners misread", wrong_unrefined, "of 36 cases")


@pytest.mark.parametrize("defect", ("caps swapped", "k swapped"))
def test_seeded_table_defects_flip_a_decision(defect):
    wrong = [(name, seed, sigma) for name, seed, sigma, _, stats, _, _ in _decisions(defect) if int(stats[0]) != ms.EXPECTED[name]]
    print(defect, "flips", len(wrong), "of 36")
    assert wrong


def _tree(v):
    while len(v) > 1:
        half = len(v) // 2
        v = [v[i] + v[i + half] for i in range(half)]
    return v[0]


def test_the_summation_order():
    """block_sum against plain Python: thread t adds its rows in ascending order, the lanes of a wave pair up at distances 32 .. 1,
    the waves add as (0 + 1) + (2 + 3) - on the rho column of a scene, in its bits.  Another wave order gives other bits."""
    sc, _, res = ms.scene_selection("curved")
    pr = res["producers"]
    args = (sc["xy"], 1000, sc["intrinsics"], pr["refined_pose"].astype(np.float32), pr["plane_H"], pr["rotation_H"], pr["avail"], 0.5)
    _, _, _, info = ms.model_gric(*args)
    x = np.where(np.isfinite(info["x"][0]) & (info["x"][0] < 2.0), info["x"][0], 2.0)
    threads = []
    for t in range(256):
        acc = 0.0
        for i in range(t, 1000, 256):
            acc = acc + x[i]
        threads.append(acc)
    w = [_tree(threads[64 * k:64 * k + 64]) for k in range(4)]
    assert info["sums"][0] == (w[0] + w[1]) + (w[2] + w[3])
    differ = 0                                              # four values can add to the same bits in two orders: not in all 12 triples
    for sigma in SIGMAS:
        straight, swapped = ms.model_gric(*args[:-1], sigma)[3]["sums"], ms.model_gric(*args[:-1], sigma, defect="wave order")[3]["sums"]
        differ += int((straight[:3] != swapped[:3]).sum())
        assert np.array_equal(straight[3:], swapped[3:])        # the counts are integers: exact in any order
    assert differ > 0
    H0 = pr["homography_H"]
    k0, k1 = mr.cam_of(sc["intrinsics"][0]), mr.cam_of(sc["intrinsics"][1])
    rows = sc["xy"].astype(np.float64)
    a = ms.pass_sums(rows, k0, k1, ms.start_state(H0, 0), ms.unit_directions(), 2.0)
    b = ms.pass_sums(rows, k0, k1, ms.start_state(H0, 0), ms.unit_directions(), 2.0, defect="wave order")
    assert not np.array_equal(a, b) and np.allclose(a, b, rtol=1e-12, atol=1e-9)


def test_edge_rules():
    """Ties and availability, a non-finite model, no model, no usable row, a NaN row, and a row exactly at its cap."""
    sc, _, res = ms.scene_selection("rotation")
    pr = res["producers"]
    xy, K = sc["xy"][:300].copy(), sc["intrinsics"]
    R = pr["rotation_H"]
    pose_e = pr["refined_pose"].astype(np.float32)
    # the plane and the rotation hold the SAME matrix: equal sums; the rotation pays for fewer parameters; with equal k as well
    # (the tie proper) the order decides
    gric, label, stats, info = ms.model_gric(xy, 300, K, pose_e, R, R, (1, 1, 1), 0.5)
    assert info["sums"][1] == info["sums"][2] and stats[0] == 2 and gric[1] - gric[2] == stats[5] > 0
    assert np.array_equal((label >> 1) & 1, (label >> 2) & 1)
    inf = np.inf
    for values, want, reversed_want in (((7.0, 7.0, 7.0), (2, 1), (0, 1)), ((7.0, 7.0, inf), (1, 0), (0, 1)), ((7.0, inf, 7.0), (2, 0), (0, 2)),
                                        ((6.0, 7.0, 7.0), (0, 2), (0, 1)), ((8.0, 7.0, 7.0), (2, 1), (1, 2)), ((inf, inf, 3.0), (2, -1), (2, -1)),
                                        ((inf, inf, inf), (-1, -1), (-1, -1))):
        assert ms.pick(np.array(values)) == want and ms.pick(np.array(values), "ties reversed") == reversed_want, values
    # every avail pattern: a model that is out has gric +inf, count 0 and no label bit; the pick is the smallest of the rest
    for bits in range(8):
        avail = [(bits >> m) & 1 for m in range(3)]
        g, lab, st, _ = ms.model_gric(xy, 300, K, pose_e, pr["plane_H"], R, avail, 0.5)
        inn = [m for m in range(3) if avail[m]]
        assert all(np.isinf(g[m]) and st[2 + m] == 0 and not ((lab >> m) & 1).any() for m in range(3) if not avail[m])
        assert all(g[m] == gric_full for m, gric_full in zip(inn, ms.model_gric(xy, 300, K, pose_e, pr["plane_H"], R, (1, 1, 1), 0.5)[0][inn]))
        if not inn:
            assert st[0] == -1 and st[6] == 1 and np.isinf(st[5]) and st[1] == 300
        else:
            assert st[0] == min(inn, key=lambda m: (g[m], -m)) and st[6] == 0 and np.isinf(st[5]) == (len(inn) == 1)
    bad = pr["plane_H"].copy()
    bad[4] = np.nan
    g, lab, st, _ = ms.model_gric(xy, 300, K, pose_e, bad, R, (1, 1, 1), 0.5)
    assert np.isinf(g[1]) and st[0] == 2 and not ((lab >> 1) & 1).any()
    g, lab, st, _ = ms.model_gric(xy, 300, K, np.full((4, 4), np.inf, dtype=np.float32), bad, bad, (1, 1, 1), 0.5)
    assert np.isinf(g).all() and st[0] == -1 and st[6] == 1 and not lab.any()
    # no usable row: status 2; a NaN row inside the count is left out of every sum and gets label 0
    for count in (0, -4):
        g, lab, st, _ = ms.model_gric(xy, count, K, pose_e, pr["plane_H"], R, (1, 1, 1), 0.5)
        assert np.isinf(g).all() and st[0] == -1 and st[1] == 0 and st[6] == 2 and not lab.any() and not st[2:5].any()
    holed = xy.copy()
    holed[17, 1] = np.nan
    g, lab, st, info = ms.model_gric(holed, 300, K, pose_e, pr["plane_H"], R, (1, 1, 1), 0.5)
    without = ms.model_gric(np.delete(xy, 17, axis=0), 299, K, pose_e, pr["plane_H"], R, (1, 1, 1), 0.5)
    assert st[1] == 299 and lab[17] == 0 and np.array_equal(st[2:5], without[2][2:5]) and np.allclose(g, without[0], rtol=1e-13)
    assert ms.model_gric(xy, 200, K, pose_e, pr["plane_H"], R, (1, 1, 1), 0.5)[1][200:].sum() == 0
    # a row exactly at its cap is NOT below it
    sigma = None                                            # e^2 / (sigma sigma) == 4.0 exactly: not every row has such a sigma
    for row in np.flatnonzero(np.isfinite(info["x"][2]) & (info["x"][2] > 0.5)):
        e2 = info["x"][2][row] * 0.25
        s = np.sqrt(e2 / 4.0)
        for cand in (s, np.nextafter(s, 0.0), np.nextafter(s, np.inf)):
            if e2 / (cand * cand) == 4.0:
                sigma = cand
        if sigma is not None:
            break
    assert sigma is not None
    one = holed[row:row + 1]
    strict = ms.model_gric(one, 1, K, pose_e, pr["plane_H"], R, (0, 0, 1), sigma)
    loose = ms.model_gric(one, 1, K, pose_e, pr["plane_H"], R, (0, 0, 1), sigma, defect="cap inclusive")
    assert strict[3]["x"][2][0] == 4.0 and strict[1][0] == 0 and strict[2][4] == 0 and loose[1][0] == 4 and loose[2][4] == 1
    assert strict[0][2] == loose[0][2]
