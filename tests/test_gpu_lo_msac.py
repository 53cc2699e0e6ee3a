"""coponerf_amd.matches.ransac_pose(score="msac", lo=K) on the MI355X (`pytest -m gpu`): cpn_ransac_score_slots, cpn_ransac_polish and
cpn_ransac_finish_lo (csrc/ransac.hip, round 24 of the header) one by one against the restatement of tests/lo_msac_ref.py (pinned
on the CPU by tests/test_lo_msac_ref.py), each fed from the restatement so that it does not depend on the kernel before it, and
the whole call.

B = 2 pairs of N = 768 rows with counts 257 and 511: a chunk boundary inside each pair, a trailing chunk of zeros, one and two
chunks in use.  40 eight-point hypotheses (not a multiple of the 256-slot tile) and 30 five-point samples (300 + K slots: a second
tile, most slots invalid); K = 1, 8, and 8 with 4 hypotheses; a pair of 7 matches beside a normal one; rel_pose given and not;
inlier_px = 0.  Every output buffer starts as NaN / 0xFF / -1 between guards.

Partials, the hypotheses' scores, the rank list, the votes, the statuses and the valid bytes are compared exactly
(tests/test_lo_msac_ref.py shows the margins that allow it).  The polish takes a sine and a cosine: a polished E is held to
lm.polish_bound, the bound of tests/test_gpu_matches.py for cpn_refine_pose per step, its score to lm.polished_score_bound of the
MEASURED difference, and the final results are the restatement's because tests/test_lo_msac_ref.py shows every fixture's winner
to lead by more than that.
"""
import functools

import numpy as np
import pytest
import torch

from coponerf_amd import _hip
from tests import lo_msac_ref as lm
from tests import matches_ref as mr
from tests import ransac_ref as rr
from tests.test_gpu_point_cloud import Guarded
from tests.test_lo_msac_ref import GPU_CONFIGS

pytestmark = pytest.mark.gpu

E_SHAPE, E_ARG = _hip.CONSTANTS["E_SHAPE"], _hip.CONSTANTS["E_ARG"]
CHUNKS = 3


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _case(config, dev):
    """The fixture of a configuration on the device and the restatement's dicts: (xy, counts, K, P or None, want)."""
    solver, Hn, kind, lo, with_rel, px, iters, short = config
    xy, counts, K, P = lm.gpu_case()
    counts = np.asarray((7, counts[1]) if short else counts, dtype=np.int32)
    return _up(xy, dev), _up(counts, dev), _up(K, dev), (_up(P, dev) if with_rel else None), lm.gpu_want(*config)


def _stack(want, key):
    return np.stack([w[key] for w in want])


def _score_slots(Em, valid, xd, cd, kd, pd, first, total, graded, px, partial):
    B, Hn = Em.shape[:2]
    _hip.call("cpn_ransac_score_slots", Em.data_ptr(), valid.data_ptr(), xd.data_ptr(), cd.data_ptr(), kd.data_ptr(),
              0 if pd is None else pd.data_ptr(), B, lm.N_GPU, Hn, first, total, graded, px, partial.ptr, _hip.stream_handle())


@functools.lru_cache(maxsize=None)
def _polished(config):
    """cpn_ransac_polish fed with the restatement's hypotheses and partials -> (E_lo (2, K, 9), valid_lo, info (2, K, 8)).
    Run once per configuration, shared, never written to."""
    solver, Hn, kind, lo, with_rel, px, iters, short = config
    dev = torch.device("cuda:0")
    xd, cd, kd, pd, want = _case(config, dev)
    Em, valid, part = (_up(_stack(want, k), dev) for k in ("E", "valid", "partial"))
    slots = Em.shape[1]
    E_lo, valid_lo, info = Guarded(2 * lo * 9, torch.float64, dev), Guarded(2 * lo, torch.uint8, dev), Guarded(2 * lo * 8, torch.float64, dev)
    _hip.call("cpn_ransac_polish", Em.data_ptr(), valid.data_ptr(), part.data_ptr(), xd.data_ptr(), cd.data_ptr(), kd.data_ptr(), 2,
              lm.N_GPU, slots, lo, iters, px, px if px > 0 else 1.0, E_lo.ptr, valid_lo.ptr, info.ptr, _hip.stream_handle())
    return E_lo.get().reshape(2, lo, 9).copy(), valid_lo.get().reshape(2, lo).copy(), info.get().reshape(2, lo, 8).copy()


# ------------------------------------------------------------------------------------------------------------- the score
@pytest.mark.parametrize("config", [c for c in GPU_CONFIGS if c[3] in (0, 8)])
def test_score_slots_against_the_restatement(dev, config):
    """The hypotheses into columns 0 .. slots - 1 of the (2, 3, slots + K + 1) partials, then the restatement's polished slots
    into columns slots .. with rel_pose's column behind them: every int32 exactly the restatement's, under the configuration's
    score and under the other one; the columns a call does not own keep their -1; the chunk beyond both counts is 0; without
    rel_pose its column is 0."""
    solver, Hn, kind, lo, with_rel, px, iters, short = config
    xd, cd, kd, pd, want = _case(config, dev)
    Em, valid, E_lo, valid_lo = (_up(_stack(want, k), dev) for k in ("E", "valid", "E_lo", "valid_lo"))
    slots, T = Em.shape[1], Em.shape[1] + lo
    for graded in (1, 0):
        if graded == (kind == "msac"):
            ref = _stack(want, "partial")
        else:
            other = lm.gpu_want(solver, Hn, "msac" if graded else "inliers", lo, with_rel, px, iters, short)
            ref = _stack(other, "partial")
            if lo:                                                  # the other score ranks, and so polishes, other slots: score these ones
                xy, counts, K, P = lm.gpu_case()
                for b in range(2):
                    n = 7 if (short and b == 0) else counts[b]
                    ref[b][:, slots:T] = lm.score(want[b]["E_lo"], want[b]["valid_lo"], xy[b], n, K[b], px, bool(graded))[:, :lo]
        partial = Guarded(2 * CHUNKS * (T + 1), torch.int32, dev)
        _score_slots(Em, valid, xd, cd, kd, pd, 0, T, graded, px, partial)
        got = partial.get().reshape(2, CHUNKS, T + 1).copy()
        assert np.array_equal(got[..., :slots], ref[..., :slots])
        if lo:
            assert (got[..., slots:] == -1).all()                   # not this call's columns
            _score_slots(E_lo, valid_lo, xd, cd, kd, pd, slots, T, graded, px, partial)
            got = partial.get().reshape(2, CHUNKS, T + 1)
        assert np.array_equal(got, ref), (graded, np.argwhere(got != ref)[:5])
        assert not got[:, 2].any() and (with_rel or not got[..., T].any())
        if graded:
            assert got.max() <= 2 ** 28 and got.astype(np.int64).sum(axis=1).max() > 2 ** 20 or px == 0.0


# ------------------------------------------------------------------------------------------------------------ the polish
@pytest.mark.parametrize("config", [c for c in GPU_CONFIGS if c[3]])
def test_polish_against_the_restatement(dev, config):
    """cpn_ransac_polish fed with the restatement's hypotheses and scores.  info - the slot of every rank, the passes made, the
    four vote counts, the status - and the valid bytes exactly; ranks beyond the valid slots and the pair of 7 matches are
    invalid with E = 0; a polished E within lm.polish_bound; its score, by cpn_ransac_score_slots, within
    lm.polished_score_bound of the measured difference."""
    solver, Hn, kind, lo, with_rel, px, iters, short = config
    xd, cd, kd, pd, want = _case(config, dev)
    E_lo, valid_lo, info = _polished(config)
    assert set(np.unique(valid_lo)) <= {0, 1} and np.isfinite(E_lo).all() and np.isfinite(info).all()
    xy, counts, K, P = lm.gpu_case()
    slots, graded = want[0]["E"].shape[0], kind == "msac"
    partial = Guarded(2 * CHUNKS * (slots + lo + 1), torch.int32, dev)
    _score_slots(_up(E_lo, dev), _up(valid_lo, dev), xd, cd, kd, pd, slots, slots + lo, int(graded), px, partial)
    scored = partial.get().reshape(2, CHUNKS, slots + lo + 1)[..., slots:slots + lo].astype(np.int64).sum(axis=1)
    worst, equal = 0.0, True
    for b, w in enumerate(want):
        n = 7 if (short and b == 0) else counts[b]
        assert np.array_equal(info[b], w["info"]), (b, info[b], w["info"])
        assert list(info[b][:, 0]) == w["ranks"] and np.array_equal(valid_lo[b], w["valid_lo"])
        assert not E_lo[b][valid_lo[b] == 0].any()
        for k in np.flatnonzero(valid_lo[b]):
            dE = float(np.abs(E_lo[b, k] - w["E_lo"][k]).max())
            bound = lm.polish_bound(w["details"][k])
            worst, equal = max(worst, dE / bound), equal and E_lo[b, k].tobytes() == w["E_lo"][k].tobytes()
            assert dE <= bound, (b, k, dE, bound)
            assert abs(np.linalg.norm(E_lo[b, k]) - 1.0) < 1e-12 and E_lo[b, k][np.abs(E_lo[b, k]).argmax()] > 0
            moved = abs(int(scored[b, k]) - int(w["sums"][slots + k]))
            may = lm.polished_score_bound(dE, w["E_lo"][k], xy[b], n, K[b], px, graded) if (dE and px > 0) else 0
            assert moved <= may, (b, k, moved, may, dE)
    print(config, "polished E: largest difference / bound", worst, "; bits equal to the restatement:", equal)
    if short:
        assert not valid_lo[0].any() and (info[0][:, 7] == 2).all() and valid_lo[1].all()
    if Hn == 4:
        assert (info[:, 4:, 7] == 2).all() and not valid_lo[:, 4:].any()


# ------------------------------------------------------------------------------------------------------------ the finish
def _pose_bound(want_pose, sigma, len0):
    bound = np.full((4, 4), rr.split_bound(sigma))
    bound[:3, 3] *= len0
    bound[3] = 0
    return bound + mr.half_ulp32(want_pose)


@pytest.mark.parametrize("config", GPU_CONFIGS)
def test_finish_lo_against_the_restatement(dev, config):
    """cpn_ransac_finish_lo fed with the restatement's hypotheses, polished slots, info and partials: the winner, the inlier
    bytes, the score, lo, stats [0 - 4] and [7] exactly - [0] the winner's inlier COUNT under either score -, the pose within
    half an fp32 ulp plus rr.split_bound as in round 20's test (and, printed, whether it IS the restatement's rounded)."""
    solver, Hn, kind, lo, with_rel, px, iters, short = config
    xd, cd, kd, pd, want = _case(config, dev)
    Em, valid, part = (_up(_stack(want, k), dev) for k in ("E", "valid", "partial"))
    E_lo, valid_lo, info = (_up(_stack(want, k), dev) for k in ("E_lo", "valid_lo", "info"))
    slots = Em.shape[1]
    pose, inlier, stats = Guarded(32, torch.float32, dev), Guarded(2 * lm.N_GPU, torch.uint8, dev), Guarded(16, torch.float64, dev)
    score, lo_out = Guarded(2, torch.int64, dev), Guarded(8, torch.float64, dev)
    _hip.call("cpn_ransac_finish_lo", Em.data_ptr(), valid.data_ptr(), E_lo.data_ptr(), valid_lo.data_ptr(), info.data_ptr(),
              part.data_ptr(), xd.data_ptr(), cd.data_ptr(), kd.data_ptr(), 0 if pd is None else pd.data_ptr(), 2, lm.N_GPU, slots, lo,
              int(kind == "msac"), px, pose.ptr, inlier.ptr, stats.ptr, score.ptr, lo_out.ptr, _hip.stream_handle())
    pose, inlier, stats = pose.get().reshape(2, 4, 4), inlier.get().reshape(2, -1), stats.get().reshape(2, 8)
    score, lo_out = score.get(), lo_out.get().reshape(2, 4)
    P = lm.gpu_case()[3]
    for b, w in enumerate(want):
        assert np.array_equal(stats[b, :5], w["stats"][:5]) and stats[b, 7] == w["stats"][7], (b, stats[b], w["stats"])
        assert np.array_equal(inlier[b], w["inlier"]) and score[b] == w["score"] and np.array_equal(lo_out[b], w["lo"])
        assert np.abs(stats[b, 5:7] - w["stats"][5:7]).max() <= 1e-9
        if w["stats"][7] == 0:
            len0 = float(np.linalg.norm(P[b][:3, 3].astype(np.float64))) if with_rel else 1.0
            err = np.abs(pose[b].astype(np.float64) - w["pose"])
            print(config, "pair", b, "pose: largest error / bound", float((err[:3] / _pose_bound(w["pose"], w["finish"]["sigma"], len0)[:3]).max()),
                  "; the restatement rounded to fp32:", pose[b].tobytes() == w["pose"].astype(np.float32).tobytes(), "; stats", stats[b],
                  "score", score[b], "lo", lo_out[b])
            assert (err <= _pose_bound(w["pose"], w["finish"]["sigma"], len0)).all() and inlier[b].sum() == stats[b, 0]
        else:
            assert pose[b].tobytes() == (P[b] if with_rel else np.eye(4, dtype=np.float32)).tobytes() and not inlier[b].any()
    if short:
        assert stats[0, 7] == 2 and stats[1, 7] == 0


# ------------------------------------------------------------------------------------------------------------- whole call
def _matches(config, dev):
    from coponerf_amd import matches as mt
    xd, cd, kd, pd, want = _case(config, dev)
    return mt.Matches(xd, None, cd), kd, pd, want


def _host(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


@pytest.mark.parametrize("config", GPU_CONFIGS)
def test_ransac_pose_whole_call(dev, config):
    """ransac_pose(score=, lo=) on the device against the restatement: nothing read on the host, the same bytes on two runs,
    the winner, the statuses, stats [0 - 4], lo and - the winner being the same - the inlier bytes exactly, the final pose the
    restatement's to round 20's bound.  The score is the restatement's exactly where a hypothesis won and within
    lm.polished_score_bound of the polish kernel's measured E difference where a polished slot did."""
    from coponerf_amd import matches as mt
    solver, Hn, kind, lo, with_rel, px, iters, short = config
    m, kd, pd, want = _matches(config, dev)
    kw = dict(hypotheses=Hn, inlier_px=px, seed=lm.SEED_GPU, solver=solver, score=kind, lo=lo, lo_iters=iters,
              lo_scale_px=None if px > 0 else 1.0)
    mt.ransac_pose(m, kd, pd, **kw)                                 # warms up
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        first, again = mt.ransac_pose(m, kd, pd, **kw), mt.ransac_pose(m, kd, pd, **kw)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    res, again = _host(first), _host(again)
    assert set(res) == {"pose", "inlier", "stats", "score", "lo"} and all(res[k].tobytes() == again[k].tobytes() for k in res)
    assert res["score"].dtype == np.int64 and res["score"].shape == (2,) and res["lo"].shape == (2, 4) and res["lo"].dtype == np.float64
    xy, counts, K, P = lm.gpu_case()
    E_lo = _polished(config)[0] if lo else None
    for b, w in enumerate(want):
        n = 7 if (short and b == 0) else counts[b]
        st = res["stats"][b]
        assert np.array_equal(st[:5], w["stats"][:5]) and st[7] == w["stats"][7], (b, st, w["stats"])
        assert np.array_equal(res["lo"][b], w["lo"]) and np.array_equal(res["inlier"][b], w["inlier"])
        if w["lo"][0]:
            k = int(w["stats"][2]) - len(w["E"])
            dE = float(np.abs(E_lo[b, k] - w["E_lo"][k]).max())
            may = lm.polished_score_bound(dE, w["E_lo"][k], xy[b], n, K[b], px, kind == "msac") if dE else 0
            assert abs(int(res["score"][b]) - w["score"]) <= may, (b, res["score"][b], w["score"], may)
        else:
            assert res["score"][b] == w["score"]
        if st[7] == 0:
            len0 = float(np.linalg.norm(P[b][:3, 3].astype(np.float64))) if with_rel else 1.0
            err = np.abs(res["pose"][b].astype(np.float64) - w["pose"])
            print(config, "pair", b, "stats", st, "score", res["score"][b], "lo", res["lo"][b], "; pose the restatement's rounded to fp32:",
                  res["pose"][b].tobytes() == w["pose"].astype(np.float32).tobytes())
            assert (err <= _pose_bound(w["pose"], w["finish"]["sigma"], len0)).all()
            assert st[0] == res["inlier"][b].sum() and (kind == "msac" or res["score"][b] == st[0])
            assert kind != "msac" or 0 < res["score"][b] <= int(st[0]) << 20
    base = lm.gpu_want(solver, Hn, kind, 0, with_rel, px, iters, short)
    assert all(res["score"][b] >= base[b]["score"] for b in range(2))                       # never below the score without lo


def test_defaults_take_the_parent_path(dev):
    """ransac_pose with its defaults against score="inliers", lo=0 spelled out, both solvers: the same three keys, the same
    bytes; and against cpn_ransac_finish_lo with K = 0 on the same counts: the same pose, inlier bytes and stats."""
    from coponerf_amd import matches as mt
    config = GPU_CONFIGS[0]
    m, kd, pd, _ = _matches(config, dev)
    for solver, Hn in (("8pt", 40), ("5pt", 30)):
        plain = _host(mt.ransac_pose(m, kd, pd, hypotheses=Hn, seed=lm.SEED_GPU, solver=solver))
        named = _host(mt.ransac_pose(m, kd, pd, hypotheses=Hn, seed=lm.SEED_GPU, solver=solver, score="inliers", lo=0, lo_iters=7,
                                     lo_scale_px=3.0))
        assert set(plain) == set(named) == {"pose", "inlier", "stats"} and all(plain[k].tobytes() == named[k].tobytes() for k in plain)
        graded = _host(mt.ransac_pose(m, kd, pd, hypotheses=Hn, seed=lm.SEED_GPU, solver=solver, score="msac"))
        assert (graded["stats"][:, 7] == 0).all() and (graded["lo"] == np.array([0, -1, -1, 0.0])).all()
        assert (graded["stats"][:, 2] < (10 if solver == "5pt" else 1) * Hn).all()


def test_keywords_pass_through_and_bad_values_raise(dev):
    """from_flows and select_pose hand score, lo, lo_iters and lo_scale_px on to ransac_pose - without them nothing changes -
    and bad values are ValueErrors that name the argument."""
    from coponerf_amd import matches as mt
    f0, f1, K, Pt, Ps = rr.flow_scene()
    flows = (_up(f0, dev), _up(f1, dev))
    Kd, Pd = _up(K, dev), _up(Ps, dev)
    kw = dict(S=32, max_cycle_px=1e9, stride=2)
    opts = {"hypotheses": 64, "seed": 0, "start": "ransac"}
    plain = mt.from_flows(flows, Kd, Pd, ransac=opts, **kw)
    lo = mt.from_flows(flows, Kd, Pd, ransac=dict(opts, score="msac", lo=4, lo_iters=2, lo_scale_px=1.5), **kw)
    assert set(plain["ransac"]) == {"pose", "inlier", "stats"} and set(lo["ransac"]) == set(plain["ransac"]) | {"score", "lo"}
    truth = {"R_true": Pt[0, :3, :3].astype(np.float64), "t_true": Pt[0, :3, 3].astype(np.float64)}
    print("from_flows errors", mr.pose_errors(plain["pose"][0].cpu().numpy(), truth), mr.pose_errors(lo["pose"][0].cpu().numpy(), truth),
          "lo", lo["ransac"]["lo"].cpu().numpy())
    assert float(lo["ransac"]["stats"][0, 7]) == 0 and max(mr.pose_errors(lo["pose"][0].cpu().numpy(), truth)) < 0.1
    chosen = mt.select_pose(lo["matches"], Kd, Pd, hypotheses=64, score="msac", lo=2)
    assert set(chosen["ransac"]) == {"pose", "inlier", "stats", "score", "lo"}
    sel = mt.from_flows(flows, Kd, Pd, select={"hypotheses": 64, "lo": 2}, **kw)
    assert "lo" in sel["select"]["ransac"]
    m = lo["matches"]
    for bad, name in (({"score": "magsac"}, "score"), ({"lo": 17}, "lo"), ({"lo": -1}, "lo"), ({"lo": 1.5}, "lo"), ({"lo_iters": -1}, "lo_iters"),
                      ({"lo": 2, "lo_scale_px": 0.0}, "lo_scale_px"), ({"lo_scale_px": float("nan")}, "lo_scale_px"),
                      ({"lo_scale_px": float("inf")}, "lo_scale_px"), ({"lo": 2, "inlier_px": 0.0}, "lo_scale_px")):
        with pytest.raises(ValueError, match=name):
            mt.ransac_pose(m, Kd, Pd, **bad)
    with pytest.raises(ValueError):
        mt.from_flows(flows, Kd, Pd, ransac={"lo_passes": 3}, **kw)
    with pytest.raises(ValueError):
        mt.select_pose(m, Kd, Pd, sweeps=3)


def test_bad_shapes_are_status_codes(dev):
    """Shapes and values the three entry points do not take come back as status codes before any launch."""
    lib = _hip.lib()
    buf = torch.zeros(4096, dtype=torch.float32, device=dev)
    p, s = buf.data_ptr(), _hip.stream_handle()
    score = lambda B, N, Hn, first, total, graded=1, px=1.0, out=p: lib.cpn_ransac_score_slots(p, p, p, p, p, p, B, N, Hn, first, total,
                                                                                               graded, px, out, s)
    polish = lambda B, N, Hn, K, iters=4, px=1.0, scale=1.0, out=p: lib.cpn_ransac_polish(p, p, p, p, p, p, B, N, Hn, K, iters, px, scale,
                                                                                          out, p, p, s)
    finish = lambda B, N, Hn, K, graded=1, px=1.0, out=p: lib.cpn_ransac_finish_lo(p, p, p, p, p, p, p, p, p, p, B, N, Hn, K, graded, px,
                                                                                   out, p, p, p, p, s)
    for args in ((0, 8, 8, 0, 8), (1, 0, 8, 0, 8), (1, 8, -1, 0, 8), (1, 8, 8, -1, 8), (1, 8, 8, 1, 8), (1, 8, 8, 0, 2 ** 20 + 1),
                 (40000, 8, 8, 0, 8), (2000, 2 ** 20, 2 ** 10, 0, 2 ** 10)):
        assert score(*args) == E_SHAPE and b"cpn_ransac_score_slots" in lib.cpn_last_error()
    for args in ((0, 8, 8, 1), (1, 0, 8, 1), (1, 8, -1, 1), (1, 8, 8, 0), (1, 8, 8, 17), (1, 8, 2 ** 20, 1), (2000, 2 ** 20, 2 ** 10, 8)):
        assert polish(*args) == E_SHAPE and b"cpn_ransac_polish" in lib.cpn_last_error()
    for args in ((0, 8, 8, 1), (1, 0, 8, 1), (1, 8, -1, 1), (1, 8, 8, -1), (1, 8, 8, 17), (1, 8, 2 ** 20, 1), (2000, 2 ** 20, 2 ** 10, 8)):
        assert finish(*args) == E_SHAPE and b"cpn_ransac_finish_lo" in lib.cpn_last_error()
    for px in (-1.0, float("nan"), float("inf")):
        assert score(1, 8, 8, 0, 8, px=px) == E_ARG and polish(1, 8, 8, 1, px=px) == E_ARG and finish(1, 8, 8, 1, px=px) == E_ARG
    assert score(1, 8, 8, 0, 8, graded=2) == E_ARG and finish(1, 8, 8, 1, graded=-1) == E_ARG
    assert polish(1, 8, 8, 1, iters=-1) == E_ARG and polish(1, 8, 8, 1, scale=0.0) == E_ARG and polish(1, 8, 8, 1, scale=float("nan")) == E_ARG
    assert score(1, 8, 8, 0, 8, out=0) == E_ARG and polish(1, 8, 8, 1, out=0) == E_ARG and finish(1, 8, 8, 1, out=0) == E_ARG
    assert score(1, 8, 0, 0, 8) == 0                                # nothing to score: nothing launched
    torch.cuda.synchronize()
    assert not bool(buf.any())                                      # nothing ran
