"""coponerf_amd.matches.homography_pose on the MI355X (`pytest -m gpu`): cpn_ransac_homographies, cpn_ransac_score_h and
cpn_ransac_finish_h (csrc/ransac_h.hip) against the restatement of tests/homography_ref.py (pinned on the CPU by
tests/test_homography_ref.py), and the whole call.

Every output buffer starts as NaN (floats) or 0xFF bytes / -1 (integers) between guard rows.  The restatement follows the kernels
operation by operation (+ - * / sqrt only), so every H is compared in its BITS; samples, validity, partial counts, the winner, the
inlier bytes, votes, Sampson counts and statuses are compared exactly (tests/test_homography_ref.py shows that no decision of the
fixtures lies within 1e-9 of its threshold); pose and twin are held to the restatement rounded to fp32 within half an ulp plus
homography_ref.decompose_bound.
"""
import numpy as np
import pytest
import torch

from coponerf_amd import _hip
from tests import homography_ref as hr
from tests import matches_ref as mr
from tests import ransac5_ref as r5
from tests import ransac_ref as rr
from tests.test_gpu_matches import pair  # noqa: F401  (the synthetic-weight model and one pair of noise photos)
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


def _host(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def _matches(xy, count, dev):
    from coponerf_amd import matches as mt
    return mt.Matches(_up(xy, dev), None, _up(np.asarray(count, dtype=np.int32), dev))


def _run_hypotheses(xy, count, K, Hn, seed, dev):
    B, N = xy.shape[:2]
    xd, cd, kd = (_up(a, dev) for a in (xy, count, K))
    H, sample, valid = Guarded(B * Hn * 9, torch.float64, dev), Guarded(B * Hn * 4, torch.int32, dev), Guarded(B * Hn, torch.uint8, dev)
    _hip.call("cpn_ransac_homographies", xd.data_ptr(), cd.data_ptr(), kd.data_ptr(), B, N, Hn, seed, H.ptr, sample.ptr, valid.ptr,
              _hip.stream_handle())
    return H.get().reshape(B, Hn, 9), sample.get().reshape(B, Hn, 4), valid.get().reshape(B, Hn)


def _run_score(Hm, valid, xy, count, K, px, dev):
    B, N = xy.shape[:2]
    Hn = Hm.shape[1]
    chunks = -(-N // CHUNK)
    hd, vd, xd, cd, kd = (_up(a, dev) for a in (Hm, valid, xy, count, K))
    partial = Guarded(B * chunks * Hn, torch.int32, dev)
    _hip.call("cpn_ransac_score_h", hd.data_ptr(), vd.data_ptr(), xd.data_ptr(), cd.data_ptr(), kd.data_ptr(), B, N, Hn, px, partial.ptr,
              _hip.stream_handle())
    return partial.get().reshape(B, chunks, Hn)


def _run_finish(Hm, valid, partial, xy, count, K, P, px, base, dev):
    B, N = xy.shape[:2]
    Hn = Hm.shape[1]
    hd, vd, pd_, xd, cd, kd = (_up(a, dev) for a in (Hm, valid, partial, xy, count, K))
    pd = None if P is None else _up(P, dev)
    pose, twin, Hout, inlier, stats = (Guarded(B * 16, torch.float32, dev), Guarded(B * 16, torch.float32, dev),
                                       Guarded(B * 9, torch.float64, dev), Guarded(B * N, torch.uint8, dev),
                                       Guarded(B * 12, torch.float64, dev))
    _hip.call("cpn_ransac_finish_h", hd.data_ptr(), vd.data_ptr(), pd_.data_ptr(), xd.data_ptr(), cd.data_ptr(), kd.data_ptr(),
              0 if pd is None else pd.data_ptr(), B, N, Hn, px, base, pose.ptr, twin.ptr, Hout.ptr, inlier.ptr, stats.ptr,
              _hip.stream_handle())
    return pose.get().reshape(B, 4, 4), twin.get().reshape(B, 4, 4), Hout.get().reshape(B, 9), inlier.get().reshape(B, N), stats.get().reshape(B, 12)


# ------------------------------------------------------------------------------------------------------------- hypotheses
@pytest.mark.parametrize("Hn", (65, 1))
def test_homographies_against_the_restatement(dev, Hn):
    """B = 6 pairs of 100 rows (homography_ref.hypotheses_case: a NaN row, three collinear points, exactly four rows, copies of one
    match, a negative count, three rows); Hn = 65 is a full workgroup of 64 and one lane of a second, Hn = 1 a single lane.
    Samples and validity exactly, every H in its bits, every element written.  Observed on the MI355X: largest
    |H - restatement| 0.0 in every pair; 13, 50, 65, 9, 0 and 0 of the 65 hypotheses are valid."""
    xy, count, K = hr.hypotheses_case()
    H, sample, valid = _run_hypotheses(xy, count, K, Hn, 0, dev)
    assert set(np.unique(valid)) <= {0, 1} and np.isfinite(H).all()
    for b in range(len(count)):
        wH, wsample, wvalid, _ = hr.hypotheses(xy[b], count[b], K[b], Hn, 0)
        assert np.array_equal(sample[b], wsample) and np.array_equal(valid[b], wvalid), b
        assert (H[b][valid[b] == 0] == 0).all()
        diff = np.abs(H[b] - wH).max()
        print("pair", b, "valid", int(valid[b].sum()), "of", Hn, "largest |H - restatement|", float(diff))
        assert H[b].tobytes() == wH.tobytes(), (b, diff)
    if Hn == 65:
        assert valid[0].sum() >= 10 and valid[1].sum() > 30 and valid[2].all() and valid[3].any()
        assert not valid[4].any() and not valid[5].any() and (sample[4] == -1).all() and ((sample[5] == -1).sum(axis=1) == 1).all()
        assert np.array_equal(sample[3], rr.draw_samples(0, Hn, 100)[0][:, :4])           # the first 4 of the 8-point's sample
        drew = (sample[0] == hr.NAN_ROW).any(axis=1)
        assert drew.any() and not valid[0][drew].any()
        line = np.isin(sample[1], (0, 1, 2)).sum(axis=1) == 3
        assert line.any() and not valid[1][line].any() and valid[1][~line].all()
        copies = (sample[3] < 50).sum(axis=1)
        assert (copies == 4).any() and not valid[3][copies >= 2].any()
        again = _run_hypotheses(xy, count, K, Hn, 0, dev)
        assert all(a.tobytes() == b.tobytes() for a, b in zip((H, sample, valid), again))
        other = _run_hypotheses(xy, count, K, Hn, 1, dev)
        assert not np.array_equal(other[1], sample)               # the seed matters


# ------------------------------------------------------------------------------------------------------------------ score
def test_score_h_against_the_restatement(dev):
    """B = 3, N = 2 CHUNK + 3 rows (three chunks, three rows in the last), counts (N, 0, CHUNK + 7), Hn = 257: a second tile of
    256 slots that holds one hypothesis; invalid slots are scattered among the valid ones.  Every partial count is exactly the
    restatement's; an invalid hypothesis and a chunk beyond the count give 0."""
    xy, count, K, Hm, valid = hr.score_case()
    assert xy.shape[1] == 2 * CHUNK + 3 and hr.CHUNK == CHUNK
    got = _run_score(Hm, valid, xy, count, K, 1.0, dev)
    for b in range(3):
        want = hr.score(Hm[b], valid[b], xy[b], count[b], K[b], 1.0)
        assert np.array_equal(got[b], want), (b, np.argwhere(got[b] != want)[:5])
        assert not got[b][:, valid[b] == 0].any()
    assert got[0].sum(axis=0).max() > 100 and got[0][2].max() <= 3 and got[0][:, 256].sum() > 0
    assert not got[1].any() and not got[2][2].any() and got[2][1].max() <= 7
    again = _run_score(Hm, valid, xy, count, K, 1.0, dev)
    assert again.tobytes() == got.tobytes()
    assert _hip.lib().cpn_ransac_score_h(0, 0, _up(xy, dev).data_ptr(), _up(count, dev).data_ptr(), _up(K, dev).data_ptr(), 3,
                                         xy.shape[1], 0, 1.0, 0, _hip.stream_handle()) == 0       # Hn == 0: nothing to do, no error


# ----------------------------------------------------------------------------------------------------------------- finish
def _pose_bound(want, dec, len0):
    """Half an fp32 ulp of the restatement's value plus decompose_bound per entry of R and of the unit translation, the
    translation's times its length; the last row is exact."""
    bound = np.full((4, 4), hr.decompose_bound(dec["s1"], dec["s3"]))
    bound[:3, 3] *= len0
    bound[3] = 0
    return bound + mr.half_ulp32(want)


@pytest.mark.parametrize("base", (0.0, hr.MIN_BASELINE))
def test_finish_h_against_the_restatement(dev, base):
    """B = 7 pairs of 1 000 rows fed with the restatement's H and counts (homography_ref.finish_case): the wall, the curved scene,
    the pure rotation, a tie that the lower index must win, every hypothesis invalid (status 1), three matches (status 2) and
    matches that do not move (status 3 at any min_baseline); with min_baseline = 0.05 the pure rotation is status 3 too and the
    wall is not.  The winner, the inlier bytes, every integer of the stats and the status exactly; sigma's and the winner's H in
    their bits; pose and twin within half an fp32 ulp plus decompose_bound.  Observed on the MI355X: the largest error / bound is
    0.90 - 0.99 and every pose and twin IS the restatement rounded to fp32, so what is left is the store's half ulp; the wall has
    320 inliers at winner 56 with votes 320 against 239, the pure rotation sigma_1 - sigma_3 = 0.0256."""
    xy, count, K, P, Hm, valid, partial = hr.finish_case()
    pose, twin, Hout, inlier, stats = _run_finish(Hm, valid, partial, xy, count, K, P, 1.0, base, dev)
    bare = _run_finish(Hm, valid, partial, xy, count, K, None, 1.0, base, dev)
    assert set(np.unique(inlier)) <= {0, 1}
    statuses = []
    for b, name in enumerate(hr.FINISH_PAIRS):
        want, wtwin, wH, winl, wstats, info = hr.finish(Hm[b], valid[b], partial[b], xy[b], count[b], K[b], 1.0, P[b], base)
        statuses.append(int(wstats[11]))
        assert np.array_equal(stats[b], wstats), (name, stats[b], wstats)                  # the sigma's too: the same bits
        assert np.array_equal(inlier[b], winl) and inlier[b].sum() == wstats[0], name
        assert Hout[b].tobytes() == wH.tobytes(), (name, np.abs(Hout[b] - wH).max())
        wbare = hr.finish(Hm[b], valid[b], partial[b], xy[b], count[b], K[b], 1.0, None, base)
        assert np.array_equal(bare[4][b], wbare[4]) and np.array_equal(bare[3][b], inlier[b])
        if wstats[11] == 0:
            len0 = float(np.linalg.norm(P[b][:3, 3].astype(np.float64)))
            for which, g, w, gb, wb in (("pose", pose[b], want, bare[0][b], wbare[0]), ("twin", twin[b], wtwin, bare[1][b], wbare[1])):
                err = np.abs(g.astype(np.float64) - w)
                bound = _pose_bound(w, info["dec"], len0)
                R = g[:3, :3].astype(np.float64)
                print(name, which, "largest error / bound", float((err[:3] / bound[:3]).max()), "; the restatement rounded to fp32:",
                      g.tobytes() == w.astype(np.float32).tobytes(), "; stats", stats[b])
                assert (err <= bound).all() and np.abs(R @ R.T - np.eye(3)).max() < 1e-6 and abs(np.linalg.det(R) - 1) < 1e-6
                assert abs(np.linalg.norm(g[:3, 3].astype(np.float64)) - len0) < 2e-7
                assert (np.abs(gb.astype(np.float64) - wb) <= _pose_bound(wb, info["dec"], 1.0)).all()
                assert np.array_equal(gb[:3, :3], g[:3, :3])
        elif wstats[11] == 3:
            assert pose[b].tobytes() == twin[b].tobytes() and not pose[b, :3, 3].any() and bare[0][b].tobytes() == pose[b].tobytes()
            err = np.abs(pose[b].astype(np.float64) - want)
            frames = hr.decompose_bound(wstats[8], wstats[9])      # infinite where H is a multiple of 1: nothing is rotated, exact
            bound = mr.half_ulp32(want) + (frames if np.isfinite(frames) else 0.0) * (np.arange(4)[:, None] < 3)
            print(name, "rotation only: largest error / bound", float((err[:3, :3] / bound[:3, :3]).max()), "; stats", stats[b])
            assert (err <= bound).all()
        else:
            assert pose[b].tobytes() == P[b].tobytes() == twin[b].tobytes() and not inlier[b].any() and not Hout[b].any()
            assert bare[0][b].tobytes() == np.eye(4, dtype=np.float32).tobytes() == bare[1][b].tobytes()
    assert (pose[:, 3] == np.array([0, 0, 0, 1], dtype=np.float32)).all() and (twin[:, 3] == pose[:, 3]).all()
    assert statuses == ([0, 0, 0, 0, 1, 2, 3] if base == 0.0 else [0, statuses[1], 3, 0, 1, 2, 3])
    i = hr.FINISH_PAIRS.index
    assert stats[i("tie"), 2] == stats[i("wall"), 2] and pose[i("tie")].tobytes() == pose[i("wall")].tobytes()
    assert stats[i("identity"), 0] == 1000 and np.array_equal(pose[i("identity")], np.eye(4, dtype=np.float32))
    none = _run_finish(Hm[:, :0], valid[:, :0], partial[..., :0], xy, count, K, P, 1.0, base, dev)
    assert (none[4][:, 11] == 2).all() and none[0].tobytes() == P.tobytes() and not none[3].any()      # Hn == 0


# ------------------------------------------------------------------------------------------------------------- whole call
def test_homography_pose_against_the_restatement(dev):
    """B = 3 (the wall, the curved scene, the pure rotation), N = 1000, 64 samples, rel_pose the curved scene's truth: every
    stat, the inlier bytes and the winner's H are the restatement's, pose and twin the restatement's within the bound.  Two runs
    give the same bytes, and a pair alone gives the bytes it gives in the batch.  THE CAPABILITY: with 64 samples the wall's pose
    is nearer to the truth than its twin (restatement: 1.03, 3.19 degrees off, the twin 10.56 in rotation; the MI355X: the same).
    Nothing is asserted about ransac_pose(solver="5pt") here; on this wall with 64 samples it ends 10.3, 50.7 degrees off."""
    from coponerf_amd import matches as mt
    named = hr.scenes()
    xy = np.stack([sc["xy"] for _, sc in named])
    Kd = _up(np.stack([sc["intrinsics"] for _, sc in named]), dev)
    P = np.stack([rr.true_pose(named[1][1])] * 3)
    Pd = _up(P, dev)
    m = _matches(xy, (1000, 1000, 1000), dev)
    res = _host(mt.homography_pose(m, Kd, Pd, hypotheses=64, inlier_px=1.0, seed=0))
    again = _host(mt.homography_pose(m, Kd, Pd, hypotheses=64, inlier_px=1.0, seed=0))
    assert set(res) == {"pose", "twin", "H", "inlier", "stats"} and all(res[k].tobytes() == again[k].tobytes() for k in res)
    for b, (name, sc) in enumerate(named):
        want, wtwin, wH, winl, wstats, info = hr.homography_pose(sc["xy"], 1000, sc["intrinsics"], P[b], 64, 1.0, 0)
        print(name, "stats", res["stats"][b], "errors", mr.pose_errors(res["pose"][b], sc) if name != "rotation" else None)
        assert np.array_equal(res["stats"][b], wstats) and wstats[11] == 0, (res["stats"][b], wstats)
        assert np.array_equal(res["inlier"][b], winl) and res["H"][b].tobytes() == wH.tobytes()
        len0 = float(np.linalg.norm(P[b][:3, 3].astype(np.float64)))
        for g, w in ((res["pose"][b], want), (res["twin"][b], wtwin)):
            assert (np.abs(g.astype(np.float64) - w) <= _pose_bound(w, info["dec"], len0)).all()
        alone = _host(mt.homography_pose(_matches(xy[b:b + 1], (1000,), dev), Kd[b:b + 1].contiguous(), Pd[b:b + 1].contiguous(),
                                         hypotheses=64))
        assert all(alone[k][0].tobytes() == res[k][b].tobytes() for k in res), name
    wall = named[0][1]
    err = mr.rotation_angle_deg(res["pose"][0, :3, :3].astype(np.float64), wall["R_true"])
    twin_err = mr.rotation_angle_deg(res["twin"][0, :3, :3].astype(np.float64), wall["R_true"])
    print("the wall at 64 samples: pose", err, "twin", twin_err)
    assert err < twin_err
    assert res["stats"][1, 0] < res["stats"][0, 0] / 4              # few inliers on the curved scene: the planarity verdict
    rot = _host(mt.homography_pose(m, Kd, None, hypotheses=64, min_baseline=hr.MIN_BASELINE))
    assert rot["stats"][2, 11] == 3 and rot["stats"][0, 11] == 0 and not rot["pose"][2, :3, 3].any()
    assert rot["pose"][2].tobytes() == rot["twin"][2].tobytes()
    idle = _host(mt.homography_pose(m, Kd, Pd, hypotheses=0))
    assert (idle["stats"][:, 11] == 2).all() and idle["pose"].tobytes() == P.tobytes() == idle["twin"].tobytes()


def test_from_flows_with_homography_reads_nothing_on_the_host(dev):
    """from_flows(..., homography={...}) on ransac_ref.flow_scene under set_sync_debug_mode("error"): the result carries the key
    `homography` with homography_pose's own tensors; without the keyword the result is the parent's, and with start="network"
    the refined pose is too; start="homography" refines from its pose where its status is 0."""
    from coponerf_amd import matches as mt
    f0, f1, K, Pt, Ps = rr.flow_scene()
    flows, Kd, Pd = (_up(f0, dev), _up(f1, dev)), _up(K, dev), _up(Ps, dev)
    kw = dict(S=32, max_cycle_px=1e9, stride=2)
    opts = {"hypotheses": 64, "inlier_px": 1.0, "seed": 0, "min_baseline": 0.0}
    mt.from_flows(flows, Kd, Pd, homography=opts, **kw)           # warms up
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = mt.from_flows(flows, Kd, Pd, homography=opts, **kw)
        plain = mt.from_flows(flows, Kd, Pd, **kw)
        started = mt.from_flows(flows, Kd, Pd, homography=dict(opts, start="homography"), **kw)
        both = mt.from_flows(flows, Kd, Pd, homography=opts, ransac={"hypotheses": 64, "start": "ransac"}, **kw)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert set(plain) == {"matches", "rel_pose", "pose", "stats", "fields"} and set(out) == set(plain) | {"homography"}
    assert set(both) == set(plain) | {"homography", "ransac"}
    assert set(out["homography"]) == {"pose", "twin", "H", "inlier", "stats"}
    own = mt.homography_pose(out["matches"], Kd, Pd, **opts)
    assert all(torch.equal(out["homography"][k], own[k]) for k in own)
    assert torch.equal(out["pose"], plain["pose"]) and torch.equal(out["stats"], plain["stats"])
    st = out["homography"]["stats"].cpu().numpy()
    print("homography stats", st)
    want = mt.refine_pose(out["matches"], Kd, out["homography"]["pose"] if st[0, 11] == 0 else Pd)
    assert torch.equal(started["pose"], want["pose"])
    for bad in ({"start": "other"}, {"start": "ransac"}, {"solver": "5pt"}, "homography"):
        with pytest.raises(ValueError):
            mt.from_flows(flows, Kd, Pd, homography=bad, **kw)
    with pytest.raises(ValueError, match="start"):
        mt.from_flows(flows, Kd, Pd, homography={"start": "homography"}, ransac={"start": "best"}, **kw)


def test_from_pair_with_homography_runs(dev, pair):  # noqa: F811
    """On the synthetic weights the flows carry no geometry: this only shows that the path runs, returns the key with
    homography_pose's shapes and a status the header names."""
    from coponerf_amd import matches as mt
    model, inp = pair
    res = mt.from_pair(model, inp, max_cycle_px=1e9, homography={})
    h = res["homography"]
    cap = 2 * 256 * 256
    for name, shape, dtype in (("pose", (1, 4, 4), torch.float32), ("twin", (1, 4, 4), torch.float32), ("H", (1, 9), torch.float64),
                               ("inlier", (1, cap), torch.uint8), ("stats", (1, 12), torch.float64)):
        assert tuple(h[name].shape) == shape and h[name].dtype == dtype, name
    st = h["stats"][0].cpu().numpy()
    print("homography stats on the synthetic pair", st)
    assert st[11] in (0.0, 1.0, 2.0, 3.0) and np.isfinite(h["pose"].cpu().numpy()).all()
    assert "homography" not in mt.from_pair(model, inp, max_cycle_px=1e9, refine=False)


def test_bad_arguments(dev):
    """Python's ValueErrors, and the entry points' status codes before any launch."""
    from coponerf_amd import matches as mt
    sc = r5.wall_scene(**r5.WALL)
    m = _matches(sc["xy"][None], (1000,), dev)
    Kd = _up(sc["intrinsics"][None], dev)
    for kw in ({"hypotheses": -1}, {"hypotheses": 2 ** 20 + 1}, {"inlier_px": float("nan")}, {"inlier_px": -1.0},
               {"min_baseline": -0.1}, {"min_baseline": float("inf")}, {"min_baseline": float("nan")}, {"seed": 2 ** 64}):
        with pytest.raises(ValueError):
            mt.homography_pose(m, Kd, **kw)
    with pytest.raises(ValueError):
        mt.homography_pose(m, Kd, torch.zeros(2, 4, 4, device=dev))
    with pytest.raises(ValueError):
        mt.homography_pose(m, Kd[:, :1].contiguous())
    lib = _hip.lib()
    buf = torch.zeros(4096, dtype=torch.float32, device=dev)
    p, s = buf.data_ptr(), _hip.stream_handle()
    for B, N, Hn in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (40000, 8, 8), (1, 2 ** 24 + 1, 8), (1, 8, 2 ** 20 + 1), (2000, 2 ** 20, 2 ** 10)):
        assert lib.cpn_ransac_homographies(p, p, p, B, N, Hn, 0, p, p, p, s) == E_SHAPE
        assert b"cpn_ransac_homographies" in lib.cpn_last_error()
    for B, N, Hn in ((0, 8, 8), (1, 0, 8), (1, 8, -1), (40000, 8, 8), (2000, 2 ** 20, 2 ** 10)):
        assert lib.cpn_ransac_score_h(p, p, p, p, p, B, N, Hn, 1.0, p, s) == E_SHAPE
        assert lib.cpn_ransac_finish_h(p, p, p, p, p, p, p, B, N, Hn, 1.0, 0.0, p, p, p, p, p, s) == E_SHAPE
    for px in (-1.0, float("nan"), float("inf")):
        assert lib.cpn_ransac_score_h(p, p, p, p, p, 1, 8, 8, px, p, s) == E_ARG
        assert lib.cpn_ransac_finish_h(p, p, p, p, p, p, p, 1, 8, 8, px, 0.0, p, p, p, p, p, s) == E_ARG
        assert lib.cpn_ransac_finish_h(p, p, p, p, p, p, p, 1, 8, 8, 1.0, px, p, p, p, p, p, s) == E_ARG
        assert b"min_baseline" in lib.cpn_last_error()
    assert lib.cpn_ransac_homographies(0, p, p, 1, 8, 8, 0, p, p, p, s) == E_ARG
    assert lib.cpn_ransac_score_h(p, p, p, p, p, 1, 8, 8, 1.0, 0, s) == E_ARG
    assert lib.cpn_ransac_finish_h(p, p, p, p, p, p, p, 1, 8, 8, 1.0, 0.0, p, 0, p, p, p, s) == E_ARG
    torch.cuda.synchronize()
    assert not bool(buf.any())                                   # nothing ran
