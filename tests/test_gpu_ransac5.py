"""coponerf_amd.matches.ransac_pose(solver="5pt") on the MI355X (`pytest -m gpu`): cpn_ransac_hypotheses5 (csrc/ransac5.hip)
against the restatement of tests/ransac5_ref.py (pinned on the CPU by tests/test_ransac5_ref.py), and the whole call through
round 20's score and finish kernels with 10 slots per sample.

Every output buffer starts as NaN (floats) or 0xFF bytes / -1 (integers) between guard rows.  The restatement follows the kernel
operation by operation, so E is compared in its BITS; samples, validity, counts, the winner, the inlier bytes and the statuses are
compared exactly (tests/test_ransac5_ref.py shows that no decision of the fixtures lies within 1e-9 of its threshold).
"""
import numpy as np
import pytest
import torch

from coponerf_amd import _hip
from tests import matches_ref as mr
from tests import ransac5_ref as r5
from tests import ransac_ref as rr
from tests.test_gpu_point_cloud import Guarded

pytestmark = pytest.mark.gpu

E_SHAPE, E_ARG = _hip.CONSTANTS["E_SHAPE"], _hip.CONSTANTS["E_ARG"]


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


def _run_hypotheses5(xy, count, K, Hn, seed, dev):
    B, N = xy.shape[:2]
    xd, cd, kd = (_up(a, dev) for a in (xy, count, K))
    E, sample, valid = (Guarded(B * Hn * 90, torch.float64, dev), Guarded(B * Hn * 5, torch.int32, dev),
                        Guarded(B * Hn * 10, torch.uint8, dev))
    _hip.call("cpn_ransac_hypotheses5", xd.data_ptr(), cd.data_ptr(), kd.data_ptr(), B, N, Hn, seed, E.ptr, sample.ptr, valid.ptr,
              _hip.stream_handle())
    return E.get().reshape(B, Hn, 10, 9), sample.get().reshape(B, Hn, 5), valid.get().reshape(B, Hn, 10)


@pytest.mark.parametrize("Hn", (65, 1))
def test_hypotheses5_against_the_restatement(dev, Hn):
    """B = 6 pairs of 64 rows, counts 64, 6 (redraws), 4 (below 5), 100 (beyond N), -3 and 64 with a NaN row; Hn = 65 is two
    full workgroups of 32 and one lane of a third, Hn = 1 a single lane.  Samples and validity exactly, every E in its bits,
    every element written (no NaN, no 0xFF left).  Observed on the MI355X: largest |E - restatement| 0.0 in every pair; 276 of the
    650 slots of pair 0 are valid, 246 of the pair with the NaN row."""
    xy, count, K = r5.hypotheses5_case()
    E, sample, valid = _run_hypotheses5(xy, count, K, Hn, 0, dev)
    assert set(np.unique(valid)) <= {0, 1} and np.isfinite(E).all()
    for b in range(len(count)):
        wE, wsample, wvalid, _ = r5.hypotheses5(xy[b], count[b], K[b], Hn, 0)
        assert np.array_equal(sample[b], wsample) and np.array_equal(valid[b], wvalid), b
        assert (E[b][valid[b] == 0] == 0).all()
        diff = np.abs(E[b] - wE).max()
        print("pair", b, "valid slots", int(valid[b].sum()), "largest |E - restatement|", float(diff))
        assert E[b].tobytes() == wE.tobytes(), (b, diff)
    if Hn == 65:
        n = np.clip(count, 0, 64)
        assert valid[0].sum() > 100 and valid[1].sum() > 100 and not valid[2].any() and not valid[4].any()
        assert (sample[2] == -1).sum(axis=1).min() == 1 and (sample[4] == -1).all()        # four rows: four drawn; none: none
        for b in (0, 1, 3, 5):
            assert ((sample[b] >= 0) & (sample[b] < n[b])).all() and all(len(set(r)) == 5 for r in sample[b].tolist())
        assert np.array_equal(sample[0], rr.draw_samples(0, Hn, 64)[0][:, :5])           # the first 5 of the 8-point's sample
        # a count beyond N is N: pair 3 is pair 0
        assert E[3].tobytes() == E[0].tobytes() and sample[3].tobytes() == sample[0].tobytes() and valid[3].tobytes() == valid[0].tobytes()
        # the NaN row: the samples that drew it are invalid, and no other one is
        drew = (sample[5] == r5.NAN_ROW).any(axis=1)
        assert drew.any() and not drew.all() and not valid[5][drew].any() and np.array_equal(valid[5][~drew], valid[0][~drew])
        assert E[5][~drew].tobytes() == E[0][~drew].tobytes()
        again = _run_hypotheses5(xy, count, K, Hn, 0, dev)
        assert all(a.tobytes() == b.tobytes() for a, b in zip((E, sample, valid), again))
        other = _run_hypotheses5(xy, count, K, Hn, 1, dev)
        assert not np.array_equal(other[1], sample)               # the seed matters


def test_ransac_pose_5pt_against_the_restatement(dev):
    """B = 2 (the wall and the noisy scene), N = 1000, 64 samples = 640 slots, rel_pose the truth: stats [0 - 4] and [7], the
    inlier bytes and the winner are the restatement's, the pose is the restatement's rounded to fp32.  Two runs give the same
    bytes, and a pair alone gives the bytes it gives in the batch.  Observed on the MI355X: 694 inliers, slot 461 of 262 valid
    (the wall; with 64 samples its pose is 10.28, 50.74 degrees off) and 681 inliers, slot 102 of 294 valid, 0.212, 0.989 degrees
    off (the noisy scene), as on the CPU."""
    from coponerf_amd import matches as mt
    case = r5.pose_case()
    xy = np.stack([sc["xy"] for sc, _ in case])
    Kd = _up(np.stack([sc["intrinsics"] for sc, _ in case]), dev)
    Pd = _up(np.stack([rr.true_pose(sc) for sc, _ in case]), dev)
    m = _matches(xy, (1000, 1000), dev)
    res = _host(mt.ransac_pose(m, Kd, Pd, hypotheses=64, inlier_px=1.0, seed=0, solver="5pt"))
    again = _host(mt.ransac_pose(m, Kd, Pd, hypotheses=64, inlier_px=1.0, seed=0, solver="5pt"))
    assert all(res[k].tobytes() == again[k].tobytes() for k in res)
    for b, (sc, (wpose, winl, wstats, _)) in enumerate(case):
        print("pair", b, "stats", res["stats"][b], "errors", mr.pose_errors(res["pose"][b], sc))
        assert np.array_equal(res["stats"][b, :5], wstats[:5]) and res["stats"][b, 7] == wstats[7] == 0, (res["stats"][b], wstats)
        assert np.array_equal(res["inlier"][b], winl) and res["inlier"][b].sum() == wstats[0]
        assert np.abs(res["stats"][b, 5:7] - wstats[5:7]).max() <= 1e-9
        assert res["pose"][b].tobytes() == wpose.astype(np.float32).tobytes()
        alone = _host(mt.ransac_pose(_matches(xy[b:b + 1], (1000,), dev), Kd[b:b + 1].contiguous(), Pd[b:b + 1].contiguous(),
                                     hypotheses=64, solver="5pt"))
        assert all(alone[k][0].tobytes() == res[k][b].tobytes() for k in res), b
    idle = _host(mt.ransac_pose(m, Kd, Pd, hypotheses=0, solver="5pt"))
    assert (idle["stats"][:, 7] == 2).all() and idle["pose"].tobytes() == Pd.cpu().numpy().tobytes()


def test_solver_8pt_is_the_default(dev):
    """solver="8pt" and no solver at all give the same bytes in every output."""
    from coponerf_amd import matches as mt
    sc = mr.refine_scene(**rr.NOISY)
    m = _matches(sc["xy"][None], (1000,), dev)
    Kd, Pd = _up(sc["intrinsics"][None], dev), _up(rr.stalled_start(sc)[None], dev)
    plain = _host(mt.ransac_pose(m, Kd, Pd, hypotheses=130, inlier_px=1.0, seed=3))
    named = _host(mt.ransac_pose(m, Kd, Pd, hypotheses=130, inlier_px=1.0, seed=3, solver="8pt"))
    assert plain["stats"][0, 7] == 0 and all(plain[k].tobytes() == named[k].tobytes() for k in plain)


def test_from_flows_with_the_5pt_solver_reads_nothing_on_the_host(dev):
    """from_flows(..., ransac={"solver": "5pt", "start": "ransac"}) on ransac_ref.flow_scene under
    set_sync_debug_mode("error"): the result carries the key `ransac`, and the refined pose of the pair whose rel_pose is 30
    degrees off is within 0.1 degrees of the truth (round 20's condition for the same scene)."""
    from coponerf_amd import matches as mt
    f0, f1, K, Pt, Ps = rr.flow_scene()
    flows, Kd, Pd = (_up(f0, dev), _up(f1, dev)), _up(K, dev), _up(Ps, dev)
    kw = dict(S=32, max_cycle_px=1e9, stride=2)
    opts = {"solver": "5pt", "start": "ransac", "hypotheses": 64, "inlier_px": 1.0, "seed": 0}
    mt.from_flows(flows, Kd, Pd, ransac=opts, **kw)               # warms up
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = mt.from_flows(flows, Kd, Pd, ransac=opts, **kw)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert set(out["ransac"]) == {"pose", "inlier", "stats"}
    st = out["ransac"]["stats"].cpu().numpy()
    truth = {"R_true": Pt[0, :3, :3].astype(np.float64), "t_true": Pt[0, :3, 3].astype(np.float64)}
    errs = mr.pose_errors(out["pose"][0].cpu().numpy(), truth)
    print("ransac stats", st, "errors after refinement", errs)
    assert st[0, 7] == 0 and st[0, 0] > st[0, 4] and 0 <= st[0, 2] < 640 and st[0, 3] <= 640
    assert max(errs) < 0.1
    with pytest.raises(ValueError, match="solver"):
        mt.from_flows(flows, Kd, Pd, ransac={"solver": "7pt"}, **kw)


def test_bad_arguments(dev):
    """An unknown solver and the limits on 10 hypotheses are ValueErrors; the entry point answers with status codes before any
    launch."""
    from coponerf_amd import matches as mt
    sc = mr.refine_scene(**rr.NOISY)
    m = _matches(sc["xy"][None], (1000,), dev)
    Kd = _up(sc["intrinsics"][None], dev)
    for bad in ("7pt", None, 5):
        with pytest.raises(ValueError):
            mt.ransac_pose(m, Kd, solver=bad)
    with pytest.raises(ValueError):
        mt.ransac_pose(m, Kd, hypotheses=2 ** 20 // 10 + 1, solver="5pt")       # 10 Hn > 2^20
    big = mt.Matches(torch.zeros(1, 2 ** 20, 4, device=dev), None, torch.zeros(1, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        mt.ransac_pose(big, Kd, hypotheses=2 ** 16, solver="5pt")               # chunks (10 Hn + 1) >= 2^31
    assert mt.ransac_pose(m, Kd, hypotheses=2 ** 16)["stats"].shape == (1, 8)   # what the 8-point solver still takes
    lib = _hip.lib()
    buf = torch.zeros(4096, dtype=torch.float32, device=dev)
    p, s = buf.data_ptr(), _hip.stream_handle()
    for B, N, Hn in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (40000, 8, 8), (1, 2 ** 24 + 1, 8), (1, 8, 2 ** 20 // 10 + 1), (2000, 2 ** 20, 2 ** 7)):
        assert lib.cpn_ransac_hypotheses5(p, p, p, B, N, Hn, 0, p, p, p, s) == E_SHAPE
        assert b"cpn_ransac_hypotheses5" in lib.cpn_last_error()
    assert lib.cpn_ransac_hypotheses5(0, p, p, 1, 8, 8, 0, p, p, p, s) == E_ARG
    torch.cuda.synchronize()
    assert not bool(buf.any())                                   # nothing ran
