"""tests/homography_ref.py against independent forms, on the CPU: the numpy restatement the GPU tests of homography_pose compare the
kernels with must itself be right, a seeded defect in each of its rules must be caught, the fixtures must keep every decision at
least 1e-9 from its threshold - and the results that justify the feature: the wall's pose with few samples, the planarity verdict
on a curved scene, and the pure rotation told from a baseline.
"""
import numpy as np
import pytest

from tests import homography_ref as hr
from tests import matches_ref as mr
from tests import ransac5_ref as r5
from tests import ransac_ref as rr


# ------------------------------------------------------------------------------------------------------------ the samples
def test_sample_is_the_head_of_round_20s():
    for n in (1000, 6, 4):
        s4, got = rr.draw_samples(3, 200, n, k=4)
        assert (got == 4).all() and np.array_equal(s4, rr.draw_samples(3, 200, n, k=8)[0][:, :4])
        assert all(len(set(r)) == 4 for r in s4.tolist()) and s4.min() >= 0 and s4.max() < n
    s, got = rr.draw_samples(3, 50, 3, k=4)
    assert (got == 3).all() and (s[:, 3] == -1).all()


def _systems(sc, Hn, seed):
    k0, k1 = mr.cam_of(sc["intrinsics"][0]), mr.cam_of(sc["intrinsics"][1])
    Hm, sample, valid, info = hr.hypotheses(sc["xy"], len(sc["xy"]), sc["intrinsics"], Hn, seed, defect="no sample test")
    pts = rr.normalised(sc["xy"][sample], k0, k1)
    return Hm, valid != 0, hr.system(*pts), pts


@pytest.mark.parametrize("name", ("wall", "curved"))
def test_null_vector_against_numpy_svd(name):
    """The null vector of the 8 x 9 system against numpy's SVD at round 20's bound NULL_OPS E / (sigma_8 / sigma_1), error over
    bound as tests/test_ransac_ref.py forms it.  Observed: none of 2 000 hypotheses of the wall or of the curved scene below
    sigma_8 / sigma_1 = 1e-5; the largest error / bound 0.0012 and 0.0015."""
    Hm, valid, A, _ = _systems(dict(hr.scenes())[name], 2000, 0)
    _, sv, Vt = np.linalg.svd(A)
    ratio, want = sv[:, 7] / sv[:, 0], Vt[:, 8]
    err = np.minimum(np.abs(Hm - want).max(axis=1), np.abs(Hm + want).max(axis=1))
    keep = ratio >= 1e-5
    bound = rr.NULL_OPS * rr.E / ratio
    print("below the cut", float((~keep).mean()), "; largest error / bound", float((err[keep] / bound[keep]).max()), "; invalid",
          int((~valid).sum()))
    assert (~keep).mean() <= 0.05
    # a valid hypothesis has det > 0, which the SVD's vector has up to its sign; an invalid one above the cut has det <= 0 only
    # where the four matches admit no orientation-preserving homography: it is 0, and finite
    assert (err[keep & valid] <= bound[keep & valid]).all() and valid[keep].mean() > 0.5
    assert np.isfinite(Hm).all() and (Hm[~valid] == 0).all()
    norm = np.sqrt((Hm[valid] ** 2).sum(axis=1))
    assert np.abs(norm - 1).max() < 1e-14 and (np.linalg.det(Hm[valid].reshape(-1, 3, 3)) > 0).all()


def test_samples_map_onto_themselves():
    """|a x H b|_inf of the four sampled matches <= SAMPLE_OPS E kappa |a| |b|, kappa = sigma_1 / sigma_8 of the system.
    Observed: the largest value / bound 1.3e-4 over 2 000 hypotheses of the wall."""
    Hm, valid, A, (a0, a1, b0, b1) = _systems(r5.wall_scene(**r5.WALL), 2000, 0)
    sv = np.linalg.svd(A, compute_uv=False)
    kappa = sv[:, 0] / sv[:, 7]
    M = Hm.reshape(-1, 3, 3)
    a = np.stack((a0, a1, np.ones_like(a0)), -1)                    # (H, 4, 3)
    b = np.stack((b0, b1, np.ones_like(b0)), -1)
    hb = np.einsum("hij,hkj->hki", M, b)
    cross = np.abs(np.cross(a, hb)).max(axis=2)
    bound = hr.SAMPLE_OPS * hr.E * kappa[:, None] * np.linalg.norm(a, axis=2) * np.linalg.norm(b, axis=2)
    worst = float((cross[valid] / bound[valid]).max())
    print("largest |a x H b| / bound", worst)
    assert valid.sum() > 1000 and worst <= 1.0


def test_degenerate_samples_fail_the_rank_test():
    sc = r5.wall_scene(**r5.WALL)
    k0, k1 = mr.cam_of(sc["intrinsics"][0]), mr.cam_of(sc["intrinsics"][1])
    copies = np.repeat(sc["xy"][5:6], 4, axis=0)
    line = hr.collinear_rows()[:4]
    for rows in (copies, line):
        _, valid = hr.null_vector(hr.system(*rr.normalised(rows[None], k0, k1)))
        assert not valid[0]
    assert hr.null_vector(hr.system(*rr.normalised(sc["xy"][None, :4], k0, k1)))[1][0]
    assert hr.null_vector(hr.system(*rr.normalised(line[None], k0, k1)), defect="no rank test")[1][0]      # the check above bites


def test_hypotheses_case_holds_what_it_says():
    """The six pairs: the NaN row's samples alone are invalid in pair 0; in pair 1 exactly the samples with all three collinear
    rows fail; pair 2's samples are the same four rows; pair 3's samples with two copies fail, and some hold four; pairs 4 and 5
    have nothing valid.  Observed valid of 65: 13, 50, 65, 9, 0, 0."""
    xy, counts, K = hr.hypotheses_case()
    res = [hr.hypotheses(xy[b], counts[b], K[b], 65, 0) for b in range(6)]
    print("valid", [int(r[2].sum()) for r in res])
    Hm, sample, valid, info = res[0]
    drew = (sample == hr.NAN_ROW).any(axis=1)
    assert drew.any() and not drew.all() and not valid[drew].any() and valid[~drew].sum() >= 10
    Hm, sample, valid, info = res[1]
    line = np.isin(sample, (0, 1, 2)).sum(axis=1) == 3
    assert line.any() and not line.all() and not valid[line].any() and valid[~line].all()
    assert (sample < 6).all()
    Hm, sample, valid, info = res[2]
    assert (np.sort(sample, axis=1) == np.arange(4)).all() and valid.all()
    Hm, sample, valid, info = res[3]
    copies = (sample < 50).sum(axis=1)
    assert (copies == 4).any() and not valid[copies >= 2].any() and valid[copies < 2].any() and sample.max() >= 64
    for b in (4, 5):
        assert not res[b][2].any() and (res[b][0] == 0).all()
    assert (res[4][1] == -1).all() and ((res[5][1] == -1).sum(axis=1) == 1).all()
    for Hm, sample, valid, info in res:
        assert (Hm[valid == 0] == 0).all()
        v = valid != 0
        if v.any():                                                 # margins: determinant and third components clear of 0
            assert info["det"][v].min() > 1e-9 and info["m2"][v].min() > 1e-9 and info["w2"][v].min() > 1e-9


def test_a_homography_that_maps_its_sample_behind_the_camera_is_invalid():
    sc = r5.wall_scene(**r5.WALL)
    Hm, sample, valid, info = hr.hypotheses(sc["xy"], 1000, sc["intrinsics"], 2000, 0)
    loose = hr.hypotheses(sc["xy"], 1000, sc["intrinsics"], 2000, 0, defect="no sample test")[2]
    behind = (loose != 0) & (valid == 0)
    print("hypotheses that map their own sample behind a camera:", int(behind.sum()), "of", int((loose != 0).sum()))
    assert behind.any() and ((info["m2"][behind] <= 0).any(axis=1) | (info["w2"][behind] <= 0).any(axis=1)).all()


# ------------------------------------------------------------------------------------------------------------- the score
def _textbook_inliers(h, xy, K, px):
    """Pixel homographies K0 H inv(K1) and its inverse on homogeneous pixels, numpy's own inverse: another form of the rule."""
    K0, K1 = K[0][:3, :3].astype(np.float64), K[1][:3, :3].astype(np.float64)
    G = K0 @ h.reshape(3, 3) @ np.linalg.inv(K1)
    x0 = np.concatenate((xy[:, :2].astype(np.float64), np.ones((len(xy), 1))), 1)
    x1 = np.concatenate((xy[:, 2:].astype(np.float64), np.ones((len(xy), 1))), 1)
    f, r = x1 @ G.T, x0 @ np.linalg.inv(G).T * np.sign(np.linalg.det(G))
    with np.errstate(all="ignore"):
        d0 = np.linalg.norm(f[:, :2] / f[:, 2:] - x0[:, :2], axis=1)
        d1 = np.linalg.norm(r[:, :2] / r[:, 2:] - x1[:, :2], axis=1)
        return (f[:, 2] > 0) & (r[:, 2] > 0) & (d0 <= px) & (d1 <= px)


def test_score_counts_against_the_textbook_form():
    """The partial counts of the score case against pixel homographies and numpy's inverse; every transfer distance of the case is
    at least 1e-9 px from the threshold and every third component at least 1e-9 from 0.  Two seeded defects of the rule change the
    counts.  Observed margins: 3.1e-6 px and 1.3e-6."""
    xy, counts, K, Hm, valid = hr.score_case()
    assert Hm.shape == (3, 257, 9) and valid[0, 256] == 1 and valid[0, 255] == 0 and valid[0].sum() > 50
    partial = hr.score(Hm[0], valid[0], xy[0], counts[0], K[0], 1.0)
    assert partial.shape == (3, 257) and partial.dtype == np.int32 and partial[2].max() <= 3
    on = valid[0] != 0
    margin, depth = hr.threshold_margin(Hm[0][on], xy[0], K[0], 1.0)
    print("score case: margin", margin, "px; smallest third component", depth)
    assert margin >= hr.MARGIN and depth >= 1e-9
    want = np.array([_textbook_inliers(h, xy[0], K[0], 1.0).sum() if o else 0 for h, o in zip(Hm[0], on)])
    assert np.array_equal(partial.sum(axis=0), want) and want.max() > 100
    assert not hr.score(Hm[1], valid[1], xy[1], counts[1], K[1], 1.0).any()                 # count 0
    part = hr.score(Hm[2], valid[2], xy[2], counts[2], K[2], 1.0)
    assert not part[2].any() and part[1].max() <= 7
    assert np.array_equal(part.sum(axis=0), [_textbook_inliers(h, xy[2][:counts[2]], K[2], 1.0).sum() if o else 0 for h, o in zip(Hm[2], on)])
    # the seeded defects are caught ("no w2 test" cannot show here: with det H > 0 and a forward transfer within the threshold
    # w_2 is det H / m_2 > 0 up to the error - test_w2_is_asked_for has the matrix on which it shows)
    for defect in ("forward only", "adjugate transposed"):
        assert not np.array_equal(hr.score(Hm[0], valid[0], xy[0], counts[0], K[0], 1.0, defect=defect).sum(axis=0), want), defect


def test_w2_is_asked_for():
    """A homography whose backward map puts a match behind camera 1 while both distances are within the threshold: without
    w_2 > 0 it would count."""
    K = np.stack((mr.pinhole(200.0, 256),) * 2)
    h = np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.5, 0.0, -1.0])            # b -> b / (0.5 b0 - 1): an involution up to scale
    b = np.array([4.0, 0.3])
    m = h.reshape(3, 3) @ np.array([b[0], b[1], 1.0])
    a = m[:2] / m[2]
    xy = np.array([[a[0] * 200 + 128, a[1] * 200 + 128, b[0] * 200 + 128, b[1] * 200 + 128]], dtype=np.float32)
    d0, m2, d1, w2 = hr.distances(h[None], xy, K)
    assert m2[0, 0] > 0 and w2[0, 0] < 0 and d0[0, 0] < 1e-3 and d1[0, 0] < 1e-3
    assert not hr.inliers(h[None], xy, K, 1.0)[0, 0] and hr.inliers(h[None], xy, K, 1.0, defect="no w2 test")[0, 0]


# ---------------------------------------------------------------------------------------------------------- decomposition
def _planes():
    sc = mr.refine_scene()
    yield sc["R_true"], sc["t_true"], np.array([0.25, -0.1, 1.0]), 3.0
    yield mr.rodrigues((0.2, -1.0, 0.4), 47.0), np.array([0.1, -0.7, 0.7]), np.array([0.0, 0.0, 1.0]), 2.0
    yield mr.rodrigues((1.0, 0.1, 0.0), 3.0), np.array([0.0, 0.3, 1.0]), np.array([1.0, 0.2, 0.5]), 1.5
    yield np.eye(3), np.array([1.0, 0.0, 0.0]), np.array([0.6, 0.0, 0.8]), 4.0


def test_decomposition_returns_the_known_plane_and_pose():
    """Exact H = R + t n^T / d at four scales: every candidate satisfies Hs = R + T N^T with R a rotation, and the true
    (R, t / d, n) is among the four, all at decompose_bound (from the conditioning 1 / (sigma_1^2 - sigma_3^2) and the gaps to
    sigma_2) plus 64 E for the fixture's own roundings.  |T| = sigma_1 - sigma_3 is held to the same bound.  Observed: the largest
    error / bound 0.0017."""
    worst = 0.0
    for R, t, n, d in _planes():
        n = n / np.linalg.norm(n)
        H = R + np.outer(t, n) / d
        for scale in (1.0, 0.37, 2.9e3, 1.0 / np.sqrt((H ** 2).sum())):
            dec = hr.decompose((scale * H).reshape(9))
            assert dec["finite"] and "R" in dec
            bound = hr.decompose_bound(dec["s1"], dec["s3"]) + 64 * hr.E
            sv = np.linalg.svd(H, compute_uv=False)
            worst = max(worst, abs(dec["s1"] - sv[0] / sv[1]) / bound, abs(dec["s3"] - sv[2] / sv[1]) / bound)
            found = np.inf
            for Rc, Tc, Nc in hr.candidates(dec):
                worst = max(worst, np.abs(dec["Hs"] - (Rc + np.outer(Tc, Nc))).max() / bound, np.abs(Rc @ Rc.T - np.eye(3)).max() / bound,
                            abs(np.linalg.det(Rc) - 1) / bound, abs(np.linalg.norm(Nc) - 1) / bound,
                            abs(np.linalg.norm(Tc) - (dec["s1"] - dec["s3"])) / bound)
                found = min(found, max(np.abs(Rc - R).max(), np.abs(Tc - t / d / sv[1]).max(), np.abs(Nc - n).max()))
            worst = max(worst, found / bound)
    print("decomposition: largest error / bound", worst)
    assert worst <= 1.0


def test_rotation_only_rule():
    R = mr.rodrigues((0.3, 1.0, -0.2), 12.0)
    for h in (R.reshape(9), 0.2 * R.reshape(9), np.eye(3).reshape(9) / np.sqrt(3.0)):
        dec = hr.decompose(h, 1e-12)
        assert "Rn" in dec and dec["finite"] and np.abs(dec["Rn"] - h.reshape(3, 3) / np.cbrt(np.linalg.det(h.reshape(3, 3)))).max() < 1e-14
    dec = hr.decompose(np.eye(3).reshape(9) / np.sqrt(3.0), 0.0)
    assert "Rn" in dec and dec["s1"] == 1.0 and dec["s3"] == 1.0   # min_baseline = 0: only an exactly rotation-only H


# --------------------------------------------------------------------------------------------------------------- the finish
def _run_finish(b, min_baseline=0.0, rel=True, defect=None):
    xy, counts, K, P, Hm, valid, partial = hr.finish_case()
    return hr.finish(Hm[b], valid[b], partial[b], xy[b], counts[b], K[b], 1.0, P[b] if rel else None, min_baseline, defect)


def test_fixtures_keep_their_decisions_clear_of_the_threshold():
    """Every transfer distance of the finish case and of the three scenes at 1 024 hypotheses is at least 1e-9 px from inlier_px,
    every third component and every N . b of a winner's inliers at least 1e-9 from 0, the Sampson residuals of the candidates'
    essential matrices at least 1e-9 px from the threshold, and no winner is tied but the one that ties on purpose.  Observed:
    distances 7.4e-6 px or more, third components 9.5e-9 or more (the curved scene at 1 024 hypotheses), |N . b| 1.1e-4 or more."""
    xy, counts, K, P, Hm, valid, partial = hr.finish_case()
    for b, name in enumerate(hr.FINISH_PAIRS):
        on = valid[b] != 0
        if not on.any() or counts[b] < 4:
            continue
        margin, depth = hr.threshold_margin(Hm[b][on], xy[b], K[b], 1.0)
        pose, twin, Hout, inlier, stats, info = _run_finish(b)
        top = np.sort(np.where(on, info["sums"], -1))[::-1]
        print(name, "margin", margin, "third", depth, "top", top[:2], "status", stats[11], "small N.b", info.get("small_nb"))
        assert margin >= hr.MARGIN and depth >= 1e-9
        assert (top[0] == top[1]) == (name in ("tie", "identity"))
        if stats[11] == 0:
            assert info["small_nb"] >= 1e-9
            assert rr.threshold_margin(np.stack(info["dec"]["E"]), xy[b], K[b], 1.0) >= rr.MARGIN
    for name, _ in hr.scenes():
        sc, (pose, twin, Hout, inlier, stats, info) = hr.scene_result(name)
        on = info["valid"] != 0
        margin, depth = hr.threshold_margin(info["H"][on], sc["xy"], sc["intrinsics"], 1.0)
        top = np.sort(np.where(on, info["sums"], -1))[::-1]
        print(name, "1024: margin", margin, "third", depth, "top", top[:2], "small N.b", info["small_nb"])
        assert margin >= hr.MARGIN and depth >= 1e-9 and top[0] > top[1] and info["small_nb"] >= 1e-9
        assert rr.threshold_margin(np.stack(info["dec"]["E"]), sc["xy"], sc["intrinsics"], 1.0) >= rr.MARGIN


def test_the_lower_index_wins_the_tie():
    pose, twin, Hout, inlier, stats, info = _run_finish(hr.FINISH_PAIRS.index("tie"))
    ref = _run_finish(hr.FINISH_PAIRS.index("wall"))
    w = int(ref[4][2])
    assert stats[2] == w and stats[0] == ref[4][0] and info["sums"][(w + 7) % 64] == info["sums"][w] and (w + 7) % 64 > w
    last = _run_finish(hr.FINISH_PAIRS.index("tie"), defect="last on ties")[4]
    assert last[2] == (w + 7) % 64                                  # the seeded defect is caught
    assert pose.tobytes() == ref[0].tobytes()


def test_statuses_of_the_finish():
    xy, counts, K, P, Hm, valid, partial = hr.finish_case()
    i = hr.FINISH_PAIRS.index
    pose, twin, Hout, inlier, stats, _ = _run_finish(i("invalid"))
    assert stats[11] == 1 and stats[1] == 1000 and not stats[[0, 2, 3, 4, 5, 6, 7, 8, 9, 10]].any() and not inlier.any() and not Hout.any()
    assert pose.astype(np.float32).tobytes() == P[0].tobytes() == twin.astype(np.float32).tobytes()
    pose, twin, Hout, inlier, stats, _ = _run_finish(i("few"))
    assert stats[11] == 2 and not stats[:11].any() and not inlier.any() and pose.astype(np.float32).tobytes() == P[0].tobytes()
    pose, twin, Hout, inlier, stats, _ = _run_finish(i("few"), rel=False)
    assert stats[11] == 2 and np.array_equal(pose, np.eye(4)) and np.array_equal(twin, np.eye(4))
    pose, twin, Hout, inlier, stats, _ = hr.finish(Hm[0][:0], valid[0][:0], partial[0][:, :0], xy[0], counts[0], K[0], 1.0, P[0])
    assert stats[11] == 2                                           # no hypotheses
    pose, twin, Hout, inlier, stats, _ = _run_finish(i("identity"))
    assert stats[11] == 3 and stats[0] == 1000 == inlier.sum() and stats[8] == 1 and stats[9] == 1 and stats[10] == 0
    assert np.array_equal(pose, np.eye(4)) and np.array_equal(twin, pose) and not stats[4:8].any()
    assert np.abs(Hout - np.eye(3).reshape(9)).max() < 1e-15
    for name in ("wall", "rotation"):
        pose, twin, Hout, inlier, stats, _ = _run_finish(i(name), rel=False)
        assert stats[11] == 0 and abs(np.linalg.norm(pose[:3, 3]) - 1) < 1e-14 and abs(np.linalg.norm(twin[:3, 3]) - 1) < 1e-14
        sv = np.linalg.svd(Hout.reshape(3, 3), compute_uv=False)
        assert abs(sv[1] - 1) < 1e-14 and np.linalg.det(Hout.reshape(3, 3)) > 0 and inlier.sum() == stats[0]
        assert abs(stats[8] - sv[0]) < 1e-13 and abs(stats[9] - sv[2]) < 1e-13
    pose, twin, Hout, inlier, stats, _ = _run_finish(i("wall"))
    want = np.linalg.norm(P[0][:3, 3].astype(np.float64))
    assert abs(np.linalg.norm(pose[:3, 3]) - want) < 1e-12          # rel_pose's length, and nothing else of it


def _vote_and_pick(defect=None):
    """On the wall at 1 024 hypotheses: is the pose the truth's candidate, and the twin the other u's?"""
    sc = r5.wall_scene(**r5.WALL)
    pose, twin, Hout, inlier, stats, info = hr.homography_pose(sc["xy"], 1000, sc["intrinsics"], None, 1024, 1.0, 0, defect=defect)
    return mr.rotation_angle_deg(pose[:3, :3], sc["R_true"]), mr.rotation_angle_deg(twin[:3, :3], sc["R_true"]), stats, info


def test_vote_picks_the_true_candidate_on_the_wall():
    """1 024 hypotheses, seed 0.  Measured: 548 inliers of 1 000 (runner-up 532); votes 395 / 153 / 0 / 548 in the header's
    candidate order; the pose 0.286 degrees (rotation) and 0.245 degrees (translation direction) off the truth, the twin 10.369
    degrees off in rotation - the pose the 8-point solver and the few-sample 5-point solver fall into; Sampson inliers 695 and 693."""
    err, twin_err, stats, info = _vote_and_pick()
    print("pose", err, "twin", twin_err, "stats", stats, "votes", info["votes"], "samp", info["samp"])
    assert err < 1.0 < 5.0 < twin_err and stats[4] == stats[0] == 548 and stats[5] < stats[4] and stats[11] == 0
    assert sorted(info["votes"][:2]) + sorted(info["votes"][2:]) == [153, 395, 0, 548]
    swapped = _vote_and_pick(defect="twins swapped")               # the seeded defects are caught
    assert swapped[0] > 5.0 and swapped[1] < 1.0
    on_a = _vote_and_pick(defect="vote on a")
    assert not np.array_equal(on_a[3]["votes"], info["votes"])


@pytest.mark.parametrize("Hn", (16, 64, 256, 1024))
def test_wall_pose_is_nearer_to_the_truth_than_its_twin(Hn):
    """The capability: with 16, 64, 256 and 1 024 samples and seeds 0, 1, 2 the chosen pose is nearer to the truth than the twin in
    rotation.  Measured (rotation, translation direction off the truth in degrees; the twin's rotation): 16 samples 1.91, 4.13
    (10.63); 4.28, 3.11 (10.10); 1.22, 0.86 (10.35).  64 samples 1.03, 3.19 (10.56); 0.36, 2.08 (10.04); 0.32, 2.44 (10.52).
    256 samples 0.48, 2.13 (10.54); 0.21, 0.46 (10.47); 0.84, 2.20 (10.43).  1 024 samples 0.29, 0.25 (10.37); 0.21, 0.46
    (10.47); 0.10, 0.39 (10.28).  ransac_pose(solver="5pt") with 64 samples on this wall ends 10.3, 50.7 degrees off."""
    sc = r5.wall_scene(**r5.WALL)
    for seed in (0, 1, 2):
        pose, twin, Hout, inlier, stats, info = hr.homography_pose(sc["xy"], 1000, sc["intrinsics"], None, Hn, 1.0, seed)
        err, twin_err = mr.rotation_angle_deg(pose[:3, :3], sc["R_true"]), mr.rotation_angle_deg(twin[:3, :3], sc["R_true"])
        print(Hn, seed, "pose", mr.pose_errors(pose, sc), "twin", twin_err, "stats", stats)
        assert stats[11] == 0 and err < twin_err


def test_few_inliers_on_the_curved_scene_are_the_planarity_verdict():
    """stats[0] of the homography on the curved scene is below a quarter of the 8-point solver's on the same matches.  Measured:
    39 against 684."""
    sc, (pose, twin, Hout, inlier, stats, info) = hr.scene_result("curved")
    eight = rr.recovery_case()[2][2]
    print("homography", stats[0], "8-point", eight[0])
    assert stats[0] < eight[0] / 4 and stats[11] == 0


def test_rotation_scene_has_no_baseline():
    """sigma_1 - sigma_3 of the pure rotation is below the wall's (measured: 0.0086 against 0.2398; singular values 1.0074, 1,
    0.9989; 537 inliers, the nearest rotation 0.33 degrees off the truth), and with min_baseline above it the status is 3 and the
    translation 0."""
    _, (_, _, _, _, wall, _) = hr.scene_result("wall")
    sc, (pose, twin, Hout, inlier, stats, info) = hr.scene_result("rotation")
    print("rotation", stats, "wall", wall[10])
    assert stats[11] == 0 and stats[10] < hr.MIN_BASELINE < wall[10] and stats[0] > 500
    sc, (pose, twin, Hout, inlier, st3, info) = hr.scene_result("rotation", min_baseline=hr.MIN_BASELINE)
    err = mr.rotation_angle_deg(pose[:3, :3], sc["R_true"])
    print("rotation only: status", st3[11], "rotation error", err)
    assert st3[11] == 3 and not pose[:3, 3].any() and np.array_equal(pose, twin) and np.array_equal(st3[:4], stats[:4])
    assert np.array_equal(st3[8:11], stats[8:11]) and not st3[4:8].any() and err < 1.0
    assert np.abs(pose[:3, :3] @ pose[:3, :3].T - np.eye(3)).max() < 1e-14 and np.linalg.det(pose[:3, :3]) > 0
    assert hr.scene_result("wall", min_baseline=hr.MIN_BASELINE)[1][4][11] == 0
