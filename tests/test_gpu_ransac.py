"""coponerf_amd.matches.ransac_pose on the MI355X (`pytest -m gpu`): the three kernels of csrc/ransac.hip one by one against the
restatement of tests/ransac_ref.py (pinned on the CPU by tests/test_ransac_ref.py), each fed from the restatement so that it
does not depend on the kernel before it, and the whole call.

Every output buffer starts as NaN (floats) or 0xFF bytes / -1 (integers) between guard rows.  Samples, validity, counts, the
winner, the inlier bytes and the statuses are compared exactly: tests/test_ransac_ref.py shows that no decision of these
fixtures lies within 1e-9 of its threshold.  E and the pose are held to the bounds of tests/ransac_ref.py.
"""
import numpy as np
import pytest
import torch

from coponerf_amd import _hip
from tests import matches_ref as mr
from tests import ransac_ref as rr
from tests.test_gpu_point_cloud import Guarded

pytestmark = pytest.mark.gpu

E_SHAPE, E_ARG = _hip.CONSTANTS["E_SHAPE"], _hip.CONSTANTS["E_ARG"]
CHUNK = _hip.CONSTANTS["RANSAC_CHUNK"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _run_hypotheses(xy, count, K, Hn, seed, dev):
    B, N = xy.shape[:2]
    xd, cd, kd = (_up(a, dev) for a in (xy, count, K))
    E, sample, valid = Guarded(B * Hn * 9, torch.float64, dev), Guarded(B * Hn * 8, torch.int32, dev), Guarded(B * Hn, torch.uint8, dev)
    _hip.call("cpn_ransac_hypotheses", xd.data_ptr(), cd.data_ptr(), kd.data_ptr(), B, N, Hn, seed, E.ptr, sample.ptr, valid.ptr,
              _hip.stream_handle())
    return E.get().reshape(B, Hn, 9), sample.get().reshape(B, Hn, 8), valid.get().reshape(B, Hn)


def _run_score(Em, valid, xy, count, K, P, px, dev):
    B, N = xy.shape[:2]
    Hn = Em.shape[1]
    chunks = -(-N // CHUNK)
    ed, vd, xd, cd, kd = (_up(a, dev) for a in (Em, valid, xy, count, K))
    pd = None if P is None else _up(P, dev)
    partial = Guarded(B * chunks * (Hn + 1), torch.int32, dev)
    _hip.call("cpn_ransac_score", ed.data_ptr(), vd.data_ptr(), xd.data_ptr(), cd.data_ptr(), kd.data_ptr(),
              0 if pd is None else pd.data_ptr(), B, N, Hn, px, partial.ptr, _hip.stream_handle())
    return partial.get().reshape(B, chunks, Hn + 1)


def _run_finish(Em, valid, partial, xy, count, K, P, px, dev):
    B, N = xy.shape[:2]
    Hn = Em.shape[1]
    ed, vd, pd_, xd, cd, kd = (_up(a, dev) for a in (Em, valid, partial, xy, count, K))
    pd = None if P is None else _up(P, dev)
    pose, inlier, stats = Guarded(B * 16, torch.float32, dev), Guarded(B * N, torch.uint8, dev), Guarded(B * 8, torch.float64, dev)
    _hip.call("cpn_ransac_finish", ed.data_ptr(), vd.data_ptr(), pd_.data_ptr(), xd.data_ptr(), cd.data_ptr(), kd.data_ptr(),
              0 if pd is None else pd.data_ptr(), B, N, Hn, px, pose.ptr, inlier.ptr, stats.ptr, _hip.stream_handle())
    return pose.get().reshape(B, 4, 4), inlier.get().reshape(B, N), stats.get().reshape(B, 8)


# ------------------------------------------------------------------------------------------------------------- hypotheses
@pytest.mark.parametrize("Hn", (130, 1))
def test_hypotheses_against_the_restatement(dev, Hn):
    """B = 6 pairs of 64 rows, counts 64, 9, 5, 100, -3 and 64 with a NaN row; Hn = 130 is two full waves and a partial one in
    three workgroups, Hn = 1 a single lane.  Samples and validity exactly; E within NULL_OPS 2^-53 / (sigma_8 / sigma_1) of the
    restatement's wherever sigma_8 / sigma_1 >= 1e-5, and - as for the 5-point kernel, which shares the elimination
    (csrc/epipolar_system.h) - every E has the restatement's bits.  Observed on the MI355X: no hypothesis of these 64-row pairs
    lies below the cut."""
    xy, count, K = rr.hypotheses_case()
    E, sample, valid = _run_hypotheses(xy, count, K, Hn, 0, dev)
    assert set(np.unique(valid)) <= {0, 1}
    worst, equal, below = 0.0, True, 0
    for b in range(len(count)):
        wE, wsample, wvalid = rr.hypotheses(xy[b], count[b], K[b], Hn, 0)
        assert np.array_equal(sample[b], wsample) and np.array_equal(valid[b], wvalid), b
        assert np.isfinite(E[b]).all() and (E[b][valid[b] == 0] == 0).all()
        on = np.flatnonzero(wvalid)
        if len(on):
            k0, k1 = mr.cam_of(K[b][0]), mr.cam_of(K[b][1])
            sv = np.linalg.svd(rr.system(*rr.normalised(xy[b][wsample[on]], k0, k1)), compute_uv=False)
            ratio = sv[:, 7] / sv[:, 0]
            keep = ratio >= 1e-5
            below += int((~keep).sum())
            err = np.abs(E[b][on] - wE[on]).max(axis=1)
            if keep.any():
                worst = max(worst, float((err[keep] * ratio[keep] / (rr.NULL_OPS * rr.E)).max()))
            equal = equal and E[b].tobytes() == wE.tobytes()
    print("Hn", Hn, "E: largest error / bound", worst, "; below the cut", below, "; bits equal to the restatement:", equal)
    assert worst <= 1.0 and equal
    if Hn == 130:
        n = np.clip(count, 0, 64)
        assert valid[0].sum() > 100 and valid[1].sum() > 100 and not valid[2].any() and not valid[4].any()
        assert (sample[2] == -1).sum(axis=1).min() == 3 and (sample[4] == -1).all()        # five rows: five drawn; none: none
        for b in (0, 1, 3, 5):
            assert ((sample[b] >= 0) & (sample[b] < n[b])).all() and all(len(set(r)) == 8 for r in sample[b].tolist())
        # a count beyond N is N: pair 3 is pair 0
        assert E[3].tobytes() == E[0].tobytes() and sample[3].tobytes() == sample[0].tobytes() and valid[3].tobytes() == valid[0].tobytes()
        # the NaN row: the hypotheses that drew it are invalid, and no other one is
        drew = (sample[5] == rr.NAN_ROW).any(axis=1)
        assert drew.any() and not drew.all() and np.array_equal(valid[5] != 0, (valid[0] != 0) & ~drew)
        assert E[5][~drew].tobytes() == E[0][~drew].tobytes()
        again = _run_hypotheses(xy, count, K, Hn, 0, dev)
        assert all(a.tobytes() == b.tobytes() for a, b in zip((E, sample, valid), again))
        other = _run_hypotheses(xy, count, K, Hn, 1, dev)
        assert not np.array_equal(other[1], sample)               # the seed matters


# ------------------------------------------------------------------------------------------------------------------ score
@pytest.mark.parametrize("Hn", (65, 257))
def test_score_against_the_restatement(dev, Hn):
    """B = 3, N = CHUNK + 1 rows (two chunks, one row in the second), counts (CHUNK + 1, 0, 7).  Hn = 65: a full wave, one more
    hypothesis and the extra slot; Hn = 257: a second tile of 256 slots that holds one hypothesis and the extra slot.  The
    partial counts, summed on the host, are exactly the restatement's; an invalid hypothesis counts 0; without rel_pose the
    extra slot is 0 and the pointer is not read."""
    xy, count, K, P, Em, valid = rr.score_case(Hn)
    assert xy.shape[1] == CHUNK + 1 == rr.CHUNK + 1
    got = _run_score(Em, valid, xy, count, K, P, 1.0, dev)
    bare = _run_score(Em, valid, xy, count, K, None, 1.0, dev)
    for b in range(3):
        want = rr.score(Em[b], valid[b], xy[b], count[b], K[b], 1.0, P[b])
        assert np.array_equal(got[b].sum(axis=0), want.sum(axis=0)) and np.array_equal(got[b], want), b
        assert (got[b][:, 3] == 0).all()
        assert np.array_equal(bare[b][:, :-1], want[:, :-1]) and (bare[b][:, -1] == 0).all()
    assert got[0].sum(axis=0).max() > 100 and got[0][1].max() == 1 and not got[1].any() and got[2].sum(axis=0).max() <= 7
    none = _run_score(Em[:, :0], valid[:, :0], xy, count, K, P, 1.0, dev)           # no hypotheses: the extra slot alone
    assert np.array_equal(none[..., 0], got[..., -1])


# ----------------------------------------------------------------------------------------------------------------- finish
def test_finish_against_the_restatement(dev):
    """B = 4 pairs of 1 000 rows fed with the restatement's E and counts: the noisy scene, the tie fixture (every hypothesis
    reaches n: the lowest index wins), every hypothesis invalid (status 1), seven matches (status 2).  The winner, the inlier
    bytes, stats [0 - 4] and [7] exactly; the pose within half an fp32 ulp plus split_bound; the rotation orthonormal.
    Observed on the MI355X: the largest error / bound is 0.85 (noisy scene, column norms 0.7100, 0.7042, 0.0014) and 0.88 (tie
    fixture); both poses ARE the restatement's rounded to fp32, so what is left is the store's half ulp."""
    xy, count, K, P, Em, valid, partial = rr.finish_case()
    pose, inlier, stats = _run_finish(Em, valid, partial, xy, count, K, P, 1.0, dev)
    bare = _run_finish(Em, valid, partial, xy, count, K, None, 1.0, dev)
    assert set(np.unique(inlier)) <= {0, 1}
    for b in range(4):
        want, winl, wstats, info = rr.finish(Em[b], valid[b], partial[b], xy[b], count[b], K[b], 1.0, P[b])
        assert np.array_equal(stats[b, :5], wstats[:5]) and stats[b, 7] == wstats[7], (b, stats[b], wstats)
        assert np.array_equal(inlier[b], winl), b
        assert np.abs(stats[b, 5:7] - wstats[5:7]).max() <= 1e-9
        if wstats[7] == 0:
            len0 = float(np.linalg.norm(P[b][:3, 3].astype(np.float64)))
            bound = np.full((4, 4), rr.split_bound(info["sigma"]))
            bound[:3, 3] *= len0
            bound[3] = 0
            bound += mr.half_ulp32(want)
            err = np.abs(pose[b].astype(np.float64) - want)
            R = pose[b, :3, :3].astype(np.float64)
            print("pair", b, "pose: largest error / bound", float((err[:3] / bound[:3]).max()), "; sigma", info["sigma"],
                  "; the restatement rounded to fp32:", pose[b].tobytes() == want.astype(np.float32).tobytes(), "; stats", stats[b])
            assert (err <= bound).all() and np.abs(R @ R.T - np.eye(3)).max() < 1e-6 and abs(np.linalg.det(R) - 1) < 1e-6
            assert abs(np.linalg.norm(pose[b, :3, 3].astype(np.float64)) - len0) < 2e-7
            assert inlier[b].sum() == stats[b, 0]
            wb = rr.finish(Em[b], valid[b], partial[b], xy[b], count[b], K[b], 1.0, None)
            assert np.array_equal(bare[2][b, :5], wb[2][:5]) and bare[2][b, 4] == -1 and not bare[2][b, 5:].any()
            assert np.array_equal(bare[1][b], inlier[b]) and abs(np.linalg.norm(bare[0][b, :3, 3].astype(np.float64)) - 1) < 2e-7
            assert np.array_equal(bare[0][b, :3, :3], pose[b, :3, :3])
        else:
            assert pose[b].tobytes() == P[b].tobytes() and not inlier[b].any()
            assert bare[0][b].tobytes() == np.eye(4, dtype=np.float32).tobytes() and bare[2][b, 7] == wstats[7]
    assert (pose[:, 3] == np.array([0, 0, 0, 1], dtype=np.float32)).all()
    assert stats[0, 7] == 0 and stats[1, 7] == 0 and stats[2, 7] == 1 and stats[3, 7] == 2
    assert stats[1, 2] == 0 and stats[1, 0] == 1000                 # the tie goes to the lowest index
    assert stats[3, 4] == -1 and not stats[3, :4].any() and stats[2, 1] == 1000
    none = _run_finish(Em[:, :0], valid[:, :0], np.ascontiguousarray(partial[..., -1:]), xy, count, K, P, 1.0, dev)
    assert (none[2][:, 7] == 2).all() and none[0].tobytes() == P.tobytes() and not none[1].any()      # Hn == 0


# ------------------------------------------------------------------------------------------------------------- whole call
def _matches(xy, count, dev):
    from coponerf_amd import matches as mt
    return mt.Matches(_up(xy, dev), None, _up(np.asarray(count, dtype=np.int32), dev))


def _host(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def test_ransac_pose_recovers_the_stalled_start_on_the_device(dev):
    """The CPU recovery case (tests/test_ransac_ref.py) through ransac_pose and cpn_refine_pose on the device, in a batch of 3
    (the noisy scene, the tie fixture, the noisy scene cut to 500 matches): two runs give the same bytes, a pair alone gives the
    bytes it gives in the batch, refine_pose from rel_pose ends more than 25 degrees off, RANSAC within 5, refine_pose from
    RANSAC's pose within 1e-3 degrees of refine_pose from the truth, stats [0] > stats [4].  Observed on the MI355X (rotation,
    translation direction, degrees): refine_pose from rel_pose 32.0846, 31.4923; RANSAC 0.3649, 0.7136 with 684 inliers against
    rel_pose's 6; refine_pose from RANSAC's pose 0.030089, 0.056293; refine_pose from the truth 0.030090, 0.056295."""
    from coponerf_amd import matches as mt
    sc, start, (wpose, winl, wstats, _) = rr.recovery_case()
    exact = mr.refine_scene(**rr.EXACT)
    xy = np.stack((sc["xy"], exact["xy"], sc["xy"]))
    count = (1000, 1000, 500)
    Kd, Pd = _up(np.stack([sc["intrinsics"]] * 3), dev), _up(np.stack([start] * 3), dev)
    m = _matches(xy, count, dev)
    res = _host(mt.ransac_pose(m, Kd, Pd, hypotheses=1024, inlier_px=1.0, seed=0))
    again = _host(mt.ransac_pose(m, Kd, Pd, hypotheses=1024, inlier_px=1.0, seed=0))
    assert all(res[k].tobytes() == again[k].tobytes() for k in res)
    for b in range(3):
        alone = _host(mt.ransac_pose(_matches(xy[b:b + 1], count[b:b + 1], dev), Kd[b:b + 1].contiguous(), Pd[b:b + 1].contiguous()))
        assert all(alone[k][0].tobytes() == res[k][b].tobytes() for k in res), b
    assert res["pose"].shape == (3, 4, 4) and res["inlier"].shape == (3, 1000) and res["stats"].shape == (3, 8)
    assert res["inlier"].dtype == np.uint8 and res["stats"].dtype == np.float64 and res["pose"].dtype == np.float32
    assert np.array_equal(res["stats"][0, :5], wstats[:5]) and res["stats"][0, 7] == 0 and np.array_equal(res["inlier"][0], winl)
    assert not res["inlier"][2, 500:].any() and res["stats"][2, 1] == 500
    got = mr.pose_errors(res["pose"][0], sc)

    def refined(P):
        return mt.refine_pose(m, Kd, P.contiguous(), iters=10, scale_px=2.0)["pose"].cpu().numpy()[0]

    stalled = mr.pose_errors(refined(Pd), sc)
    after = mr.pose_errors(refined(_up(res["pose"], dev)), sc)
    best = mr.pose_errors(refined(_up(np.stack([rr.true_pose(sc)] * 3), dev)), sc)
    print("stalled", stalled, "ransac", got, "refined", after, "from the truth", best, "stats", res["stats"])
    assert min(stalled) > 25.0 and max(got) <= 5.0
    assert abs(after[0] - best[0]) <= 1e-3 and abs(after[1] - best[1]) <= 1e-3
    assert res["stats"][0, 0] > res["stats"][0, 4] >= 0
    bare = _host(mt.ransac_pose(m, Kd))                             # without rel_pose: the same rotation, |t| = 1, stats [4] = -1
    assert np.array_equal(bare["pose"][:, :3, :3], res["pose"][:, :3, :3]) and (bare["stats"][:, 4] == -1).all()
    assert np.array_equal(bare["inlier"], res["inlier"])
    idle = _host(mt.ransac_pose(m, Kd, Pd, hypotheses=0))
    assert (idle["stats"][:, 7] == 2).all() and idle["pose"].tobytes() == Pd.cpu().numpy().tobytes()


def test_from_flows_with_ransac_reads_nothing_on_the_host(dev):
    """from_flows(..., ransac={...}) under set_sync_debug_mode("error"); the result has the key `ransac` only when asked;
    start="best" refines pair 0 (rel_pose 30 degrees off: 0 inliers against RANSAC's) from RANSAC's pose and pair 1 (rel_pose
    the truth: a tie) from rel_pose."""
    from coponerf_amd import matches as mt
    f0, f1, K, Pt, Ps = rr.flow_scene()
    flows = (_up(np.concatenate((f0, f0)), dev), _up(np.concatenate((f1, f1)), dev))
    Kd, Pd = _up(np.concatenate((K, K)), dev), _up(np.concatenate((Ps, Pt)), dev)
    kw = dict(S=32, max_cycle_px=1e9, stride=2)
    opts = {"hypotheses": 64, "inlier_px": 1.0, "seed": 0, "start": "best"}
    mt.from_flows(flows, Kd, Pd, ransac=opts, **kw)               # warms up
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        best = mt.from_flows(flows, Kd, Pd, ransac=opts, **kw)
        plain = mt.from_flows(flows, Kd, Pd, **kw)
        from_ransac = mt.from_flows(flows, Kd, Pd, ransac=dict(opts, start="ransac"), **kw)
        network = mt.from_flows(flows, Kd, Pd, ransac={"hypotheses": 64}, **kw)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert set(plain) == {"matches", "rel_pose", "pose", "stats", "fields"} and set(best) == set(plain) | {"ransac"}
    assert set(best["ransac"]) == {"pose", "inlier", "stats"}
    st = best["ransac"]["stats"].cpu().numpy()
    n = best["matches"].count.cpu().numpy()
    print("kept", n, "ransac stats", st)
    assert (st[:, 7] == 0).all() and st[0, 0] > st[0, 4] and st[1, 0] <= st[1, 4] and (n > 200).all()
    assert tuple(best["ransac"]["inlier"].shape) == (2, 2 * 32 * 32)
    assert torch.equal(network["pose"], plain["pose"]) and torch.equal(network["stats"], plain["stats"])
    assert torch.equal(best["pose"][0], from_ransac["pose"][0]) and torch.equal(best["pose"][1], plain["pose"][1])
    assert not torch.equal(best["pose"][0], plain["pose"][0])
    truth = {"R_true": Pt[0, :3, :3].astype(np.float64), "t_true": Pt[0, :3, 3].astype(np.float64)}
    errs = [mr.pose_errors(best["pose"][b].cpu().numpy(), truth) for b in range(2)]
    print("errors after refinement", errs, "; without ransac", mr.pose_errors(plain["pose"][0].cpu().numpy(), truth))
    assert max(errs[0]) < 0.1 and max(errs[1]) < 0.1
    for bad in ({"start": "other"}, {"sweeps": 3}, "best"):
        with pytest.raises(ValueError):
            mt.from_flows(flows, Kd, Pd, ransac=bad, **kw)
    with pytest.raises(ValueError):
        mt.ransac_pose(best["matches"], Kd, Pd[:1].contiguous())
    with pytest.raises(ValueError):
        mt.ransac_pose(best["matches"], Kd, Pd, inlier_px=float("nan"))
    with pytest.raises(ValueError):
        mt.ransac_pose(best["matches"], Kd, Pd, hypotheses=-1)


def test_bad_shapes_are_status_codes(dev):
    """Shapes and values the kernels do not take come back as status codes before any launch."""
    lib = _hip.lib()
    buf = torch.zeros(4096, dtype=torch.float32, device=dev)
    p, s = buf.data_ptr(), _hip.stream_handle()
    for B, N, Hn in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (40000, 8, 8), (1, 2 ** 24 + 1, 8), (1, 8, 2 ** 20 + 1), (2000, 2 ** 20, 2 ** 10)):
        assert lib.cpn_ransac_hypotheses(p, p, p, B, N, Hn, 0, p, p, p, s) == E_SHAPE
        assert b"cpn_ransac_hypotheses" in lib.cpn_last_error()
    for B, N, Hn in ((0, 8, 8), (1, 0, 8), (1, 8, -1), (40000, 8, 8), (2000, 2 ** 20, 2 ** 10)):
        assert lib.cpn_ransac_score(p, p, p, p, p, p, B, N, Hn, 1.0, p, s) == E_SHAPE
        assert lib.cpn_ransac_finish(p, p, p, p, p, p, p, B, N, Hn, 1.0, p, p, p, s) == E_SHAPE
    for px in (-1.0, float("nan"), float("inf")):
        assert lib.cpn_ransac_score(p, p, p, p, p, p, 1, 8, 8, px, p, s) == E_ARG
        assert lib.cpn_ransac_finish(p, p, p, p, p, p, p, 1, 8, 8, px, p, p, p, s) == E_ARG
    assert lib.cpn_ransac_hypotheses(0, p, p, 1, 8, 8, 0, p, p, p, s) == E_ARG
    assert lib.cpn_ransac_score(p, p, p, p, p, p, 1, 8, 8, 1.0, 0, s) == E_ARG
    assert lib.cpn_ransac_finish(p, p, p, p, p, p, p, 1, 8, 8, 1.0, 0, p, p, s) == E_ARG
    torch.cuda.synchronize()
    assert not bool(buf.any())                                   # nothing ran
