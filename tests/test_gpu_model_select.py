"""coponerf_amd.matches.refine_homography, model_gric and select_pose on the MI355X (`pytest -m gpu`): cpn_refine_homography and
cpn_model_gric (csrc/model_select.hip) against the restatement of tests/model_select_ref.py (pinned on the CPU by
tests/test_model_select_ref.py), and the whole call.

Every output buffer starts as NaN (floats) or 0xFF bytes between guard rows.  Labels, counts, the pick, statuses and the infinities
that `avail` decides are compared exactly (tests/test_model_select_ref.py shows that no x of the fixtures lies within 1e-9 of its cap
and that every decision is won by 1000 bounds); gric at model_select_ref's summation bound; one refinement pass at
model_select_ref.refine_step_bound.  THE TEN-PASS STATE is held by its recovered distance to the truth, not by a propagated bound:
a bound carried through ten nonlinear passes grows with cond(A) every pass while Gauss-Newton itself contracts the difference, so it
would say nothing; the distance to the truth of an exact scene is what the passes are for, and its tolerance
(model_select_ref.rounding_tolerance) is a first-order bound on the fp32 rounding of the coordinates.
"""
import numpy as np
import pytest
import torch

from coponerf_amd import _hip
from tests import homography_ref as hr
from tests import matches_ref as mr
from tests import model_select_ref as ms
from tests import ransac5_ref as r5
from tests import ransac_ref as rr
from tests.test_gpu_point_cloud import Guarded

pytestmark = pytest.mark.gpu

E_SHAPE, E_ARG = _hip.CONSTANTS["E_SHAPE"], _hip.CONSTANTS["E_ARG"]
COUNTS = (0, 1, 7, 255, 256, 257, 1000)                              # the stride of 256 threads and its two neighbours
NAN_ROW = 3


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _host(res):
    return {k: v.cpu().numpy() for k, v in res.items() if torch.is_tensor(v)}


def _matches(xy, count, dev):
    from coponerf_amd import matches as mt
    return mt.Matches(_up(xy, dev), None, _up(np.asarray(count, dtype=np.int32), dev))


def _scene_rows(name, n, nan_row=True):
    """The scene's 1000 rows with the rows at and beyond n filled with NaN, and (n > NAN_ROW + 1) a NaN inside the count."""
    xy = dict(hr.scenes())[name]["xy"].copy()
    xy[n:] = np.nan
    if nan_row and n > NAN_ROW + 1:
        xy[NAN_ROW, 2] = np.nan
    return xy


def _run_refine(xy, count, K, H0, mode, iters, dev, scale_px=2.0):
    B, N = xy.shape[:2]
    xd, cd, kd, hd = (_up(a, dev) for a in (xy, np.asarray(count, dtype=np.int32), K, H0))
    H, pose, stats = Guarded(B * 9, torch.float64, dev), Guarded(B * 16, torch.float32, dev), Guarded(B * 8, torch.float64, dev)
    _hip.call("cpn_refine_homography", xd.data_ptr(), cd.data_ptr(), kd.data_ptr(), hd.data_ptr(), B, N, mode, iters, scale_px, H.ptr,
              pose.ptr, stats.ptr, _hip.stream_handle())
    return H.get().reshape(B, 9).copy(), pose.get().reshape(B, 4, 4).copy(), stats.get().reshape(B, 8).copy()


def _run_gric(xy, count, K, pose_e, Hp, Hr, avail, sigma, dev):
    B, N = xy.shape[:2]
    xd, cd, kd, pd, hp, hr, ad, td = (_up(a, dev) for a in (xy, np.asarray(count, dtype=np.int32), K, np.asarray(pose_e, dtype=np.float32),
                                                            Hp, Hr, np.asarray(avail, dtype=np.uint8), ms.ln4n_table(N)))
    gric, label, stats = Guarded(B * 3, torch.float64, dev), Guarded(B * N, torch.uint8, dev), Guarded(B * 7, torch.float64, dev)
    _hip.call("cpn_model_gric", xd.data_ptr(), cd.data_ptr(), kd.data_ptr(), pd.data_ptr(), hp.data_ptr(), hr.data_ptr(), ad.data_ptr(),
              td.data_ptr(), B, N, sigma, gric.ptr, label.ptr, stats.ptr, _hip.stream_handle())
    return gric.get().reshape(B, 3).copy(), label.get().reshape(B, N).copy(), stats.get().reshape(B, 7).copy()


def _models(names):
    """(pose_e, H_plane, H_rot, avail, K) of the named scenes' restated producers at 256 hypotheses, seed 0."""
    pr = [ms.scene_selection(n)[2]["producers"] for n in names]
    return (np.stack([p["refined_pose"].astype(np.float32) for p in pr]), np.stack([p["plane_H"] for p in pr]),
            np.stack([p["rotation_H"] for p in pr]), np.stack([p["avail"] for p in pr]),
            np.stack([ms.scene_selection(n)[0]["intrinsics"] for n in names]))


NAMES = ("wall", "curved", "rotation")


def _check_gric(got, want, name):
    gric, label, stats = got
    wgric, wlabel, wstats, info = want
    assert np.array_equal(label, wlabel), name
    assert np.array_equal(stats[[0, 1, 2, 3, 4, 6]], wstats[[0, 1, 2, 3, 4, 6]]), (name, stats, wstats)
    assert np.array_equal(np.isinf(gric), np.isinf(wgric)) and (gric[np.isinf(gric)] > 0).all(), (name, gric, wgric)
    fin = np.isfinite(wgric)
    err = np.abs(gric[fin] - wgric[fin])
    assert (err <= info["bound"][fin]).all(), (name, err, info["bound"])
    if np.isfinite(wstats[5]):
        assert abs(stats[5] - wstats[5]) <= 2.0 * info["bound"].max()
    else:
        assert stats[5] == np.inf
    return float((err / info["bound"][fin]).max()) if fin.any() else 0.0, gric.tobytes() == wgric.tobytes()


# ------------------------------------------------------------------------------------------------------------------- gric
@pytest.mark.parametrize("n", COUNTS)
def test_gric_against_the_restatement(dev, n):
    """B = 3 (the wall, the curved scene, the pure rotation with their restated refined models), N = 1000, count = n for every
    pair, the rows at and beyond n NaN and (n > 4) a NaN row inside the count: labels, the counts below the caps, n_u, the pick and
    the status exactly, gric within the summation bound, every element written.  Observed on the MI355X: error / bound 0.0 in all
    21 cases - every gric has the restatement's bits, which the test then asserts: the kernel takes only + - * / sqrt in the
    restatement's order.  At n = 1000 (999 usable) the wall scores (5216.7, 4644.5, 6717.3), the curved scene (5076.2, 6677.9, 6737.6)
    and the pure rotation (5107.9, 4712.7, 4671.8) as (E, plane, rotation)."""
    xy = np.stack([_scene_rows(name, n) for name in NAMES])
    pose_e, Hp, Hr, avail, K = _models(NAMES)
    got = _run_gric(xy, (n,) * 3, K, pose_e, Hp, Hr, avail, 0.5, dev)
    for b, name in enumerate(NAMES):
        want = ms.model_gric(xy[b], n, K[b], pose_e[b], Hp[b], Hr[b], avail[b], 0.5)
        ratio, bits = _check_gric(tuple(g[b] for g in got), want, name)
        print(name, "n", n, "gric", got[0][b], "stats", got[2][b], "largest error / bound", ratio, "; the restatement's bits:", bits)
        assert bits and np.array_equal(got[2][b], want[2])
        assert want[2][1] == (n - (1 if n > NAN_ROW + 1 else 0)) and not got[1][b][n:].any()
        if n > NAN_ROW + 1:
            assert got[1][b][NAN_ROW] == 0
        assert want[2][6] == (2 if want[2][1] == 0 else 0)
    if n == 1000:
        assert [int(s[0]) for s in got[2]] == [1, 0, 2]


def test_gric_availability_and_batch(dev):
    """B = 9 in one launch: the curved scene under all eight avail patterns, and once with a NaN in the plane's H: a model that is out
    has gric +inf, count 0 and no label bit; no model in gives -1 and status 1.  Then B = 3 with counts (1000, 0, 257) over FINITE
    rows beyond the count (they must not be read): each pair equals its own result alone, and two runs give the same bytes."""
    sc, _, res = ms.scene_selection("curved")
    pr = res["producers"]
    B = 9
    avail = np.array([[(bits >> m) & 1 for m in range(3)] for bits in range(8)] + [[1, 1, 1]], dtype=np.uint8)
    Hp = np.stack([pr["plane_H"]] * B)
    Hp[8, 4] = np.nan
    xy, K = np.stack([sc["xy"]] * B), np.stack([sc["intrinsics"]] * B)
    pose_e, Hr = np.stack([pr["refined_pose"].astype(np.float32)] * B), np.stack([pr["rotation_H"]] * B)
    got = _run_gric(xy, (1000,) * B, K, pose_e, Hp, Hr, avail, 0.5, dev)
    for b in range(B):
        _check_gric(tuple(g[b] for g in got), ms.model_gric(xy[b], 1000, K[b], pose_e[b], Hp[b], Hr[b], avail[b], 0.5), b)
    assert got[2][0, 0] == -1 and got[2][0, 6] == 1 and np.isinf(got[0][0]).all() and not got[1][0].any()
    assert np.isinf(got[0][8, 1]) and not ((got[1][8] >> 1) & 1).any() and got[2][8, 3] == 0
    counts = (1000, 0, 257)
    three = tuple(a[:3] for a in (xy, K, pose_e, Hp, Hr))
    ones = np.ones((3, 3), dtype=np.uint8)
    batch = _run_gric(three[0], counts, three[1], three[2], three[3], three[4], ones, 0.5, dev)
    again = _run_gric(three[0], counts, three[1], three[2], three[3], three[4], ones, 0.5, dev)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(batch, again))
    for b in range(3):
        alone = _run_gric(*(a[b:b + 1] for a in three[:1]), counts[b:b + 1], *(a[b:b + 1] for a in three[1:]), ones[:1], 0.5, dev)
        assert all(a[0].tobytes() == g[b].tobytes() for a, g in zip(alone, batch)), b
        _check_gric(tuple(g[b] for g in batch), ms.model_gric(xy[b], counts[b], K[b], pose_e[b], Hp[b], Hr[b], ones[b], 0.5), b)
    assert batch[2][1, 6] == 2 and batch[2][2, 1] == 257 and not batch[1][2][257:].any()


# ------------------------------------------------------------------------------------------------------------- refinement
def _state_bound(step, mode):
    return ms.refine_step_bound(step, 2.0, mode)


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("n", COUNTS)
def test_refine_one_step_against_the_restatement(dev, n, mode):
    """iters = 1 on the wall's rows from homography_pose's restated winner, count = n, NaN beyond it and (n > 4) a NaN row inside:
    every entry of H within model_select_ref.refine_step_bound (operation count, sums of absolute terms, cond(A)) of the
    restatement's single step; the rows that count, the updates and the status exactly; the costs and the weights within their own
    operation counts.  n = 0 is status 2: H0 as it came, the identity, zeros.  Observed on the MI355X: error / bound 0.0 in all 12
    cases, every H has the restatement's bits (cond(A) 1.8e5 and an entry bound of 1.1e-6 at n = 1, mode 0, where two equations meet
    eight unknowns; cond(A) 38 and 4.9e-11 at n = 1000; mode 1: cond(A) 4.5, 9.7e-12).  Mode 0 takes only + - * / sqrt, so its bits
    are asserted instead of the bound; mode 1 takes a sine and a cosine in its Rodrigues step, which two libraries may round
    differently, so it keeps the bound."""
    sc, _, res = ms.scene_selection("wall")
    H0 = res["producers"]["homography_H"]
    xy = _scene_rows("wall", n)
    H, pose, stats = _run_refine(xy[None], (n,), sc["intrinsics"][None], H0[None], mode, 1, dev)
    wH, wpose, wstats, trace = ms.refine_homography(xy, n, sc["intrinsics"], H0, mode, 1, 2.0)
    assert np.array_equal(stats[0, [3, 6, 7]], wstats[[3, 6, 7]]), (stats, wstats)
    if n == 0:
        assert wstats[7] == 2 and H[0].tobytes() == H0.tobytes() and np.array_equal(pose[0], np.eye(4, dtype=np.float32))
        assert np.array_equal(stats[0], wstats)
        return
    assert wstats[7] == 0 and wstats[6] == 1 and wstats[3] == n - (1 if n > NAN_ROW + 1 else 0)
    d_delta, entry, cond = _state_bound(trace[0], mode)
    err = np.abs(H[0] - wH)
    print("n", n, "mode", mode, "one step: largest error / bound", float(err.max() / entry), "cond(A)", cond, "entry bound", entry,
          "; the restatement's bits:", H[0].tobytes() == wH.tobytes())
    assert (err <= entry).all()
    if mode == 0:
        assert H[0].tobytes() == wH.tobytes() and np.array_equal(stats[0], wstats)
    rounds = -(-n // mr.NT)
    rel = (ms.TERM_OPS_H + rounds + 8) * ms.E
    assert abs(stats[0, 0] - wstats[0]) <= rel * wstats[0]
    NP = 9 if mode == 0 else 3
    last = trace[-1]
    dirs = ms.unit_directions() if mode == 0 else ms.rotation_directions(last["H"])
    absg = ms.pass_sums(last["rows"], *last["cams"], last["H"], dirs, 2.0, magnitude=True)[NP * (NP + 1) // 2:NP * (NP + 1) // 2 + NP]
    slack = 2.0 * np.linalg.norm(absg) * d_delta               # the cost and the weights are formed at the updated state
    assert abs(stats[0, 1] - wstats[1]) <= rel * wstats[1] + slack and abs(stats[0, 2] - wstats[2]) <= rel * wstats[2] + slack
    if mode == 0:
        assert abs(np.linalg.norm(H[0]) - 1.0) < 1e-15 and np.array_equal(pose[0], np.eye(4, dtype=np.float32))
        assert abs(stats[0, 4] - wstats[4]) <= 2.0 * 3.0 * entry and abs(stats[0, 5] - wstats[5]) <= 16.0 * entry + hr.DECOMP_OPS * hr.E
    else:
        want32 = wpose.astype(np.float32)
        assert (np.abs(pose[0].astype(np.float64) - wpose) <= entry + mr.half_ulp32(wpose)).all() and np.array_equal(pose[0][3], want32[3])
        assert not pose[0][:3, 3].any() and stats[0, 5] == 0
        assert abs(stats[0, 4] - wstats[4]) <= np.degrees(2.0 * 3.0 * entry) + 1e-12


@pytest.mark.parametrize("mode", (0, 1))
def test_refine_batch_determinism_and_nothing_to_do(dev, mode):
    """B = 5 in one launch, ten passes: the wall with counts 1000, 0 and 257 over FINITE rows beyond the count (they must not be
    read), an all-zero H0 and a NaN H0 (status 2: H0 back, the identity, zeros).  Each pair equals its own result alone; two runs
    give the same bytes; iters = 0 is status 2 for every pair; the rows that count are the restatement's."""
    sc, _, res = ms.scene_selection("wall")
    H0 = np.stack([res["producers"]["homography_H"]] * 5)
    H0[3] = 0.0
    H0[4, 2] = np.nan
    xy, K = np.stack([sc["xy"]] * 5), np.stack([sc["intrinsics"]] * 5)
    counts = (1000, 0, 257, 1000, 1000)
    batch = _run_refine(xy, counts, K, H0, mode, 10, dev)
    again = _run_refine(xy, counts, K, H0, mode, 10, dev)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(batch, again))
    for b in range(5):
        alone = _run_refine(xy[b:b + 1], counts[b:b + 1], K[b:b + 1], H0[b:b + 1], mode, 10, dev)
        assert all(a[0].tobytes() == g[b].tobytes() for a, g in zip(alone, batch)), b
        wstats = ms.refine_homography(xy[b], counts[b], K[b], H0[b], mode, 10, 2.0)[2]
        assert np.array_equal(batch[2][b, [3, 6, 7]], wstats[[3, 6, 7]]), (b, batch[2][b], wstats)
    for b in (1, 3, 4):
        assert batch[2][b, 7] == 2 and not batch[2][b, :7].any() and batch[0][b].tobytes() == H0[b].tobytes()
        assert np.array_equal(batch[1][b], np.eye(4, dtype=np.float32))
    assert batch[2][0, 7] == 0 and batch[2][0, 6] == 10 and batch[2][2, 3] == 257 and batch[2][0, 1] <= batch[2][0, 0]
    idle = _run_refine(xy, counts, K, H0, mode, 0, dev)
    assert (idle[2][:, 7] == 2).all() and idle[0].tobytes() == H0.tobytes() and not idle[2][:, :7].any()


def test_refine_recovers_exact_scenes(dev):
    """Ten passes on the wall and on the pure rotation without noise, from starts 1e-2 (Frobenius) off the truth: the device ends
    within model_select_ref.rounding_tolerance of the true h and the true R, as the restatement does (the module's docstring says
    why the ten-pass state is held this way).  Observed on the MI355X: the wall ends 2.9e-9 from the true h (tolerance 3.4e-7, start
    8.5e-3), the pure rotation 1.3e-9 from the true R (tolerance 2.0e-7, start 1.0e-2); both are the restatement's own distances."""
    wall = r5.wall_scene(noise_px=0.0, outliers=0.0)
    truth = ms.wall_truth()
    rng = np.random.default_rng(1)
    d = rng.normal(size=9)
    start = truth + 1e-2 * d / np.linalg.norm(d)
    H, _, stats = _run_refine(wall["xy"][None], (1000,), wall["intrinsics"][None], start[None], 0, 10, dev)
    wH, _, wstats, trace = ms.refine_homography(wall["xy"], 1000, wall["intrinsics"], start, 0, 10, 2.0)
    tol = ms.rounding_tolerance(trace[-1], 0)
    print("wall: device", np.linalg.norm(H[0] - truth), "restatement", np.linalg.norm(wH - truth), "tolerance", tol, "stats", stats[0])
    assert np.linalg.norm(H[0] - truth) <= tol and np.array_equal(stats[0, [3, 6, 7]], wstats[[3, 6, 7]]) and stats[0, 6] == 10
    turn = hr.rotation_scene(noise_px=0.0, outliers=0.0)
    R_start = (mr.rodrigues((0.4, -1.0, 0.3), np.degrees(1e-2 / np.sqrt(2.0))) @ turn["R_true"]).reshape(9)
    R, pose, stats = _run_refine(turn["xy"][None], (1000,), turn["intrinsics"][None], R_start[None], 1, 10, dev)
    wR, _, wstats, trace = ms.refine_homography(turn["xy"], 1000, turn["intrinsics"], R_start, 1, 10, 2.0)
    tol = ms.rounding_tolerance(trace[-1], 1)
    dist = np.linalg.norm(R[0].reshape(3, 3) - turn["R_true"])
    print("rotation: device", dist, "restatement", np.linalg.norm(wR.reshape(3, 3) - turn["R_true"]), "tolerance", tol, "stats", stats[0])
    assert dist <= tol and np.array_equal(stats[0, [3, 6, 7]], wstats[[3, 6, 7]])
    assert np.array_equal(pose[0][:3, :3], R[0].reshape(3, 3).astype(np.float32)) and not pose[0][:3, 3].any()


# ------------------------------------------------------------------------------------------------------------- whole call
def _converged_bound(last_step, mode):
    """What the state after the passes have converged may differ by: Gauss-Newton maps a difference d of the state to rho d with
    rho << 1 near the minimum and adds at most the one-step bound each pass, so the fixed point moves by at most entry / (1 - rho) <=
    2 entry."""
    return 2.0 * ms.refine_step_bound(last_step, 2.0, mode)[1]


def test_select_pose_against_the_restatement(dev):
    """select_pose on the three scenes, B = 3 in one call at 256 hypotheses: `model` is the restatement's - the wall picks the plane,
    the curved scene E, the pure rotation the rotation alone -, the labels, counts and availability are the restatement's, gric within
    the summation bound of the restatement on the device's own refined models, and `pose` is the restatement's rounded to fp32 within the bound
    of the picked model: round 22's decompose_bound for the plane, round 16's step bound for E, this round's for the rotation, each
    at the converged state.  `pose` is the picked producer's own tensor.  Observed on the MI355X: gric (5222.9, 4651.3, 6724.1) for the
    wall, (5082.3, 6684.7, 6744.4) for the curved scene, (5114.1, 4719.4, 4678.6) for the pure rotation, won by 571.6, 1602.4 and
    40.9; the largest pose error / bound is 0.48, 0.86 and 0.94 and every pose IS the restatement's rounded to fp32: what is left is
    the store's half ulp."""
    from coponerf_amd import matches as mt
    named = hr.scenes()
    xy = np.stack([sc["xy"] for _, sc in named])
    Kd = _up(np.stack([sc["intrinsics"] for _, sc in named]), dev)
    P = np.stack([rr.true_pose(named[1][1])] * 3)
    m = _matches(xy, (1000, 1000, 1000), dev)
    res = mt.select_pose(m, Kd, _up(P, dev), hypotheses=256)
    assert set(res) == {"pose", "model", "gric", "label", "stats", "avail", "ransac", "refined", "homography", "plane", "rotation"}
    assert set(res["plane"]) == {"pose", "twin", "H", "inlier", "stats", "H_refined", "refine_stats"}
    again = mt.select_pose(m, Kd, _up(P, dev), hypotheses=256)
    assert all(torch.equal(res[k], again[k]) for k in ("pose", "model", "gric", "label", "stats"))
    out = _host(res)
    assert out["model"].dtype == np.int32 and out["model"].tolist() == [1, 0, 2]
    picked = (res["refined"]["pose"], res["plane"]["pose"], res["rotation"]["pose"])
    for b, (name, sc) in enumerate(named):
        want = ms.select_pose(sc["xy"], 1000, sc["intrinsics"], P[b], 256, 1.0, 0, 0.5)
        pr = want["producers"]
        assert out["model"][b] == want["model"] == ms.EXPECTED[name] and np.array_equal(out["avail"][b], want["avail"])
        assert np.array_equal(out["label"][b], want["label"]) and np.array_equal(out["stats"][b][[0, 1, 2, 3, 4, 6]], want["stats"][[0, 1, 2, 3, 4, 6]])
        assert np.array_equal(_host(res["homography"])["H"][b], pr["homography_H"])            # round 22: the winner in its bits
        assert torch.equal(res["pose"][b], picked[want["model"]][b])
        got = out["pose"][b].astype(np.float64)
        err = np.abs(got - want["pose"])
        if want["model"] == 1:
            _, _, _, trace = ms.refine_homography(sc["xy"], 1000, sc["intrinsics"], pr["homography_H"], 0, 10, 2.0)
            dH = _converged_bound(trace[-2], 0)
            dec = hr.decompose(pr["plane_H"])
            amplify = hr.decompose_bound(dec["s1"], dec["s3"]) / (hr.DECOMP_OPS * hr.E)
            bound = np.full((4, 4), hr.decompose_bound(dec["s1"], dec["s3"]) + 4.0 * amplify * dH)
            assert np.abs(_host(res["plane"])["H_refined"][b] - pr["plane_H"]).max() <= dH
        elif want["model"] == 0:
            _, _, trace = mr.refine_pose(sc["xy"], 1000, sc["intrinsics"], pr["ransac_pose"].astype(np.float32), 10, 2.0)
            bound = np.full((4, 4), 2.0 * mr.refine_step_bound(trace[-2], 2.0, 1.0)[1])
        else:
            _, _, _, trace = ms.refine_homography(sc["xy"], 1000, sc["intrinsics"], pr["homography_H"], 1, 10, 2.0)
            bound = np.full((4, 4), _converged_bound(trace[-2], 1))
        len0 = float(np.linalg.norm(P[b][:3, 3].astype(np.float64)))
        bound[:3, 3] *= max(len0, 1.0)
        bound[3] = 0.0
        bound += mr.half_ulp32(want["pose"])
        print(name, "model", out["model"][b], "gric", out["gric"][b], "margin", out["stats"][b][5], "pose: largest error / bound",
              float((err[:3] / bound[:3]).max()), "; the restatement rounded to fp32:", out["pose"][b].tobytes() == want["pose"].astype(np.float32).tobytes())
        assert (err <= bound).all()
        # the verdict on the device's OWN refined models: the restatement of cpn_model_gric on them, at the summation bound
        own = ms.model_gric(sc["xy"], 1000, sc["intrinsics"], _host(res["refined"])["pose"][b], _host(res["plane"])["H_refined"][b],
                            _host(res["rotation"])["H"][b], out["avail"][b], 0.5)
        _check_gric((out["gric"][b], out["label"][b], out["stats"][b]), own, name)
        assert out["stats"][b][5] >= 1000.0 * own[3]["bound"].max()
    none = _host(mt.select_pose(_matches(xy, (0, 0, 0), dev), Kd, _up(P, dev), hypotheses=64))
    assert (none["model"] == -1).all() and none["pose"].tobytes() == P.tobytes() and (none["stats"][:, 6] == 2).all()
    bare = _host(mt.select_pose(_matches(xy, (0, 0, 0), dev), Kd, None, hypotheses=64))
    assert bare["pose"].tobytes() == np.stack([np.eye(4, dtype=np.float32)] * 3).tobytes()


def test_from_flows_with_select_reads_nothing_on_the_host(dev):
    """from_flows(..., select={...}) on ransac_ref.flow_scene under set_sync_debug_mode("error"): the result carries the key `select`
    with select_pose's own tensors; without the keyword the result's bytes are those of the call without it; start="selected" refines
    from the selected pose where model_gric's status is 0; a second start is a ValueError.  Which model wins here is printed, not
    asserted: at 32 x 32 pixels and a focal length of 29 the two surfaces' 397 matches score (1687.9, 1626.1, 1725.3) on the MI355X
    and the plane wins by 61.9 - the parallax of this small scene is within sigma_px of a homography."""
    from coponerf_amd import matches as mt
    f0, f1, K, Pt, Ps = rr.flow_scene()
    flows, Kd, Pd = (_up(f0, dev), _up(f1, dev)), _up(K, dev), _up(Ps, dev)
    kw = dict(S=32, max_cycle_px=1e9, stride=2)
    opts = {"hypotheses": 64, "inlier_px": 1.0, "seed": 0, "sigma_px": 0.5}
    before = mt.from_flows(flows, Kd, Pd, **kw)
    mt.from_flows(flows, Kd, Pd, select=opts, **kw)              # warms up: the ln(4 n) table is built and copied once
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = mt.from_flows(flows, Kd, Pd, select=opts, **kw)
        plain = mt.from_flows(flows, Kd, Pd, **kw)
        started = mt.from_flows(flows, Kd, Pd, select=dict(opts, start="selected"), **kw)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert set(plain) == {"matches", "rel_pose", "pose", "stats", "fields"} and set(out) == set(plain) | {"select"}
    for k in ("pose", "stats"):
        assert plain[k].cpu().numpy().tobytes() == before[k].cpu().numpy().tobytes() == out[k].cpu().numpy().tobytes()
    kept = int(before["matches"].count[0])                      # the rows beyond the count are not written
    assert torch.equal(plain["matches"].count, before["matches"].count)
    assert torch.equal(plain["matches"].xy[:, :kept], before["matches"].xy[:, :kept])
    own = mt.select_pose(out["matches"], Kd, Pd, **opts)
    assert all(torch.equal(out["select"][k], own[k]) for k in ("pose", "model", "gric", "label", "stats", "avail"))
    st = out["select"]["stats"].cpu().numpy()
    print("select stats", st, "gric", out["select"]["gric"].cpu().numpy())
    assert st[0, 6] == 0 and st[0, 0] in (0.0, 1.0, 2.0)
    want = mt.refine_pose(out["matches"], Kd, out["select"]["pose"] if st[0, 6] == 0 else Pd)
    assert torch.equal(started["pose"], want["pose"])
    for bad in ({"start": "other"}, {"start": "ransac"}, {"min_baseline": 0.1}, {"solver": "3pt"}, "selected"):
        with pytest.raises(ValueError):
            mt.from_flows(flows, Kd, Pd, select=bad, **kw)
    for other in ({"ransac": {"start": "best"}}, {"homography": {"start": "homography"}}):
        with pytest.raises(ValueError, match="start"):
            mt.from_flows(flows, Kd, Pd, select={"start": "selected"}, **other, **kw)
    mt.from_flows(flows, Kd, Pd, select={"hypotheses": 64}, ransac={"hypotheses": 64, "start": "ransac"}, **kw)    # one start: fine


def test_bad_arguments(dev):
    """Python's ValueErrors, and the entry points' status codes before any launch."""
    from coponerf_amd import matches as mt
    sc, _, res = ms.scene_selection("wall")
    pr = res["producers"]
    m = _matches(sc["xy"][None], (1000,), dev)
    Kd, Hd = _up(sc["intrinsics"][None], dev), _up(pr["plane_H"][None], dev)
    Pd, Ad = _up(pr["refined_pose"].astype(np.float32)[None], dev), _up(np.ones((1, 3), dtype=np.uint8), dev)
    for kw in ({"model": "line"}, {"iters": -1}, {"scale_px": 0.0}, {"scale_px": float("nan")}, {"scale_px": float("inf")}):
        with pytest.raises(ValueError):
            mt.refine_homography(m, Kd, Hd, **kw)
    with pytest.raises(ValueError):
        mt.refine_homography(m, Kd, Hd.float())
    with pytest.raises(ValueError):
        mt.refine_homography(m, Kd, torch.zeros(2, 9, dtype=torch.float64, device=dev))
    for sigma in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            mt.model_gric(m, Kd, Pd, Hd, Hd, Ad, sigma_px=sigma)
        with pytest.raises(ValueError):
            mt.select_pose(m, Kd, sigma_px=sigma)
    with pytest.raises(ValueError):
        mt.model_gric(m, Kd, Pd, Hd, Hd, Ad.float())
    with pytest.raises(ValueError):
        mt.model_gric(m, Kd, Pd, Hd, Hd, torch.ones(1, 2, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError):
        mt.select_pose(m, Kd, solver="3pt")
    lib = _hip.lib()
    buf = torch.zeros(4096, dtype=torch.float32, device=dev)
    p, s = buf.data_ptr(), _hip.stream_handle()
    for B, N in ((0, 8), (1, 0), (40000, 8), (1, 2 ** 24 + 1)):
        assert lib.cpn_refine_homography(p, p, p, p, B, N, 0, 1, 2.0, p, p, p, s) == E_SHAPE
        assert b"cpn_refine_homography" in lib.cpn_last_error()
        assert lib.cpn_model_gric(p, p, p, p, p, p, p, p, B, N, 0.5, p, p, p, s) == E_SHAPE
        assert b"cpn_model_gric" in lib.cpn_last_error()
    for mode, iters, scale in ((2, 1, 2.0), (-1, 1, 2.0), (0, -1, 2.0), (0, 1, 0.0), (1, 1, float("nan")), (1, 1, float("inf"))):
        assert lib.cpn_refine_homography(p, p, p, p, 1, 8, mode, iters, scale, p, p, p, s) == E_ARG
    for sigma in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.cpn_model_gric(p, p, p, p, p, p, p, p, 1, 8, sigma, p, p, p, s) == E_ARG
        assert b"sigma_px" in lib.cpn_last_error()
    assert lib.cpn_refine_homography(p, p, p, 0, 1, 8, 0, 1, 2.0, p, p, p, s) == E_ARG
    assert lib.cpn_model_gric(p, p, p, p, p, p, p, 0, 1, 8, 0.5, p, p, p, s) == E_ARG
    torch.cuda.synchronize()
    assert not bool(buf.any())                                   # nothing ran
