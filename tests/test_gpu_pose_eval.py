"""coponerf_amd.matches.pose_errors / residual_stats and Evaluator(geometry=...) on the MI355X (`pytest -m gpu`): cpn_pose_errors and
cpn_residual_stats (csrc/pose_eval.hip, round 25 of the header) against the restatement of tests/pose_eval_ref.py, pinned on the
CPU by tests/test_pose_eval_ref.py, which also shows the margins that allow the exact comparisons.

cpn_residual_stats: tests/lo_msac_ref.gpu_case() - B = 2, N = 768, counts 257 and 511: more rows than threads, no multiple of 256,
NaN beyond the counts - under P = 3 poses (the truth, one 5 degrees off, one with a NaN entry), Q = 4 (0, 0.5, 0.9, 1), T = 2 (0 and
1.0); and B = 8 pairs of residuals by construction: all zero (both signs), tied, spread over 1e-12 .. 1e3 px, a NaN row inside the
count, counts 0, 1, 5 and 6, beside a pose without a translation.  Every output starts as NaN / -1 between guards.  usable, within,
status and the BITS of quant and of both sigmas are the restatement's: sigma[1]'s sum is restated in the kernel's block order
(matches_ref.block_sum), so no tolerance is needed.
cpn_pose_errors: B = 3, P = 5 with rotations of 1e-6, 0.03 and 179.9999 degrees.  The distances in their bits; the angles within 8
ulp of numpy's arctan2 (OpenCL's bound for atan2 is 6 ulp, numpy's own 1, 1 of slack).  Largest observed: see
test_pose_errors_against_the_restatement.
"""
import ctypes

import numpy as np
import pytest
import torch

from coponerf_amd import _hip
from tests import pose_eval_ref as pe
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


def _doubles(values):
    return (ctypes.c_double * len(values))(*values)


def _same_bits(got, want):
    """Equal as bit patterns (so +0 is not -0), every NaN equal to every NaN."""
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    return bool(((got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))).all())


def _stats_call(case, dev):
    """cpn_residual_stats on a fixture of pose_eval_ref with Q_GPU and THR_GPU, every output between guards -> dict of arrays and
    their raw bytes."""
    xy, counts, K, poses = pe.scene_case() if case == "scene" else pe.shear_case()
    B, N, P, Q, T = xy.shape[0], xy.shape[1], poses.shape[1], len(pe.Q_GPU), len(pe.THR_GPU)
    xd, cd, kd, pd = _up(xy, dev), _up(counts, dev), _up(K, dev), _up(poses, dev)
    out = {"usable": Guarded(B * P, torch.int32, dev), "quant": Guarded(B * P * Q, torch.float64, dev),
           "within": Guarded(B * P * T, torch.int32, dev), "sigma": Guarded(B * P * 2, torch.float64, dev),
           "status": Guarded(B * P, torch.int32, dev)}
    _hip.call("cpn_residual_stats", xd.data_ptr(), cd.data_ptr(), kd.data_ptr(), pd.data_ptr(), _doubles(pe.Q_GPU), _doubles(pe.THR_GPU),
              B, N, P, Q, T, out["usable"].ptr, out["quant"].ptr, out["within"].ptr, out["sigma"].ptr, out["status"].ptr,
              _hip.stream_handle())
    shapes = {"usable": (B, P), "quant": (B, P, Q), "within": (B, P, T), "sigma": (B, P, 2), "status": (B, P)}
    got = {k: v.get().reshape(shapes[k]).copy() for k, v in out.items()}
    return got, b"".join(got[k].tobytes() for k in sorted(got))


@pytest.mark.parametrize("case", ["scene", "shear"])
def test_residual_stats_against_the_restatement(dev, case):
    """Counts and statuses exactly, every quantile and both sigmas in their bits; the guards hold; a second call gives the same
    bytes; rows at and beyond the count are NaN and change nothing."""
    got, raw = _stats_call(case, dev)
    want = pe.want_stats(case)
    for b, w in enumerate(want):
        for key in ("usable", "within", "status"):
            assert np.array_equal(got[key][b], w[key]), (case, b, key, got[key][b], w[key])
        assert _same_bits(got["quant"][b], w["quant"]), (case, b, got["quant"][b], w["quant"])
        assert _same_bits(got["sigma"][b][:, 0], w["sigma"][:, 0]), (case, b, got["sigma"][b], w["sigma"])
        assert _same_bits(got["sigma"][b][:, 1], w["sigma"][:, 1]), (case, b, got["sigma"][b], w["sigma"])
    assert _stats_call(case, dev)[1] == raw                            # determinism
    assert {int(v) for v in got["status"].reshape(-1)} == ({0, 2} if case == "scene" else {0, 1, 2})


def test_residual_stats_wrapper_and_errors(dev):
    """matches.residual_stats returns the kernel's tensors, drops the pose axis for (B, 4, 4), and checks its arguments; the
    entry point answers P, Q or T outside 1 .. 8 with CPN_E_SHAPE and a q outside [0, 1] or a negative threshold with CPN_E_ARG,
    before any launch."""
    from coponerf_amd import matches as mt
    xy, counts, K, poses = pe.scene_case()
    m = mt.Matches(_up(xy, dev), torch.empty(2, 768, 2, device=dev), _up(counts, dev))
    kd, pd = _up(K, dev), _up(poses, dev)
    got = mt.residual_stats(m, kd, pd, q=pe.Q_GPU, thresholds=pe.THR_GPU)
    ref, _ = _stats_call("scene", dev)
    assert all(got[k].cpu().numpy().tobytes() == ref[k].tobytes() for k in ref)
    one = mt.residual_stats(m, kd, pd[:, 0].contiguous())               # q = 0.5, thresholds = 1.0
    assert one["quant"].shape == (2, 1) and one["usable"].shape == (2,) and one["sigma"].shape == (2, 2)
    assert np.array_equal(one["quant"].cpu().numpy()[:, 0], ref["quant"][:, 0, 1])
    assert np.array_equal(one["within"].cpu().numpy()[:, 0], ref["within"][:, 0, 1])
    for bad in (dict(q=()), dict(q=(0.5,) * 9), dict(q=(1.5,)), dict(q=(float("nan"),)), dict(thresholds=(-1.0,)),
                dict(thresholds=(float("inf"),)), dict(thresholds=())):
        with pytest.raises(ValueError):
            mt.residual_stats(m, kd, pd, **bad)
    with pytest.raises(ValueError):
        mt.residual_stats(m, kd, pd[:1].contiguous())
    with pytest.raises(ValueError):
        mt.residual_stats(m, kd, torch.zeros(2, 9, 4, 4, device=dev))
    with pytest.raises(RuntimeError):
        mt.residual_stats(m, kd, pd.cpu())
    fn, q, t = _hip.lib().cpn_residual_stats, _doubles((0.5,)), _doubles((1.0,))
    call = lambda P=1, Q=1, T=1, q=q, t=t, B=2, N=768: fn(16, 16, 16, 16, q, t, B, N, P, Q, T, 16, 16, 16, 16, 16, None)
    assert [call(P=0), call(P=9), call(Q=0), call(Q=9), call(T=0), call(T=9), call(B=0), call(N=0)] == [E_SHAPE] * 8
    assert [call(q=_doubles((1.5,))), call(q=_doubles((-0.1,))), call(q=_doubles((float("nan"),))), call(t=_doubles((-1.0,))),
            call(t=_doubles((float("nan"),)))] == [E_ARG] * 5
    assert b"q[0]" in (call(q=_doubles((2.0,))) and _hip.lib().cpn_last_error())
    assert fn(None, 16, 16, 16, q, t, 2, 768, 1, 1, 1, 16, 16, 16, 16, 16, None) == E_ARG
    assert _hip.lib().cpn_pose_errors(16, 16, 1, 0, 16, None) == E_SHAPE and _hip.lib().cpn_pose_errors(16, 16, 1, 9, 16, None) == E_SHAPE
    assert _hip.lib().cpn_pose_errors(16, None, 1, 1, 16, None) == E_ARG


def test_pose_errors_against_the_restatement(dev):
    """B = 3, P = 5.  The distances in their bits (a square root is exact); the angles within 8 ulp of numpy's arctan2 on the same
    float64 arguments; NaN exactly where the restatement has it.  Largest observed ratio on gfx950: 1.0 ulp (the printed figure)."""
    from coponerf_amd import matches as mt
    poses, gt = pe.errors_case()
    out = Guarded(3 * 5 * 3, torch.float64, dev)
    pd, gd = _up(poses, dev), _up(gt, dev)
    _hip.call("cpn_pose_errors", pd.data_ptr(), gd.data_ptr(), 3, 5, out.ptr, _hip.stream_handle())
    got = out.get().reshape(3, 5, 3).copy()
    want = np.stack([pe.pose_errors(poses[b], gt[b]) for b in range(3)])
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert _same_bits(got[..., 1], want[..., 1])
    ratio = pe.ulps(got[..., [0, 2]], want[..., [0, 2]])
    print(f"cpn_pose_errors: largest angle difference {ratio.max():.2f} ulp")
    assert ratio.max() <= 8.0, ratio
    assert got[0, 0, 0] > 0.0 and abs(got[0, 0, 0] - np.radians(1e-6)) < 2.0 ** -22 * np.radians(1e-6)
    wrapped = mt.pose_errors(pd, gd)
    assert wrapped.shape == (3, 5, 3) and wrapped.cpu().numpy().tobytes() == got.tobytes()
    single = mt.pose_errors(pd[:, 2].contiguous(), gd)
    assert single.shape == (3, 3) and single.cpu().numpy().tobytes() == got[:, 2].tobytes()
    with pytest.raises(ValueError):
        mt.pose_errors(pd, gd[:2].contiguous())
    with pytest.raises(ValueError):
        mt.pose_errors(torch.zeros(3, 9, 4, 4, device=dev), gd)


# ------------------------------------------------------------------------------------------------------------- Evaluator
GEOMETRY = {"S": 32, "max_cycle_px": 1e9, "stride": 2, "ransac": {"hypotheses": 64}, "select": {"hypotheses": 64}}


def _batch(seed, dev):
    """Two pairs of tests/ransac_ref.flow_scene - rel_pose 30 degrees off and the truth - with random 16 x 16 images."""
    f0, f1, K, Pt, Ps = rr.flow_scene()
    g = torch.Generator().manual_seed(seed)
    rgb, gt = (torch.rand(2, 1, 256, 3, generator=g) * 2 - 1).to(dev), (torch.rand(2, 1, 256, 3, generator=g) * 2 - 1).to(dev)
    out = {"rgb": rgb, "rel_pose": _up(np.concatenate((Ps, Pt) if seed % 2 == 0 else (Pt, Ps)), dev),
           "gt_rel_pose": _up(np.concatenate((Pt, Pt)), dev), "flow": (_up(np.concatenate((f0, f0)), dev), _up(np.concatenate((f1, f1)), dev))}
    return out, gt, _up(np.concatenate((K, K)), dev)


def test_evaluator_geometry_columns(dev):
    """Two add calls under set_sync_debug_mode("error"): no host read; the new columns equal in their bits what from_flows,
    pose_errors and residual_stats return when called apart; the built-in columns equal those of an Evaluator() fed the same
    batches; summary() carries the new keys; a missing intrinsics and an unknown key raise."""
    from coponerf_amd import matches as mt
    from coponerf_amd.evaluate import AUC_AT, COLUMNS, QUALITY, Evaluator
    batches = [_batch(0, dev), _batch(1, dev)]
    Evaluator(geometry=GEOMETRY).add(*batches[0][:2], [0.6, 0.8], intrinsics=batches[0][2])        # warms up
    ev, plain = Evaluator(geometry=GEOMETRY, capacity=2), Evaluator(capacity=2)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for out, gt, K in batches:
            ev.add(out, gt, [0.6, 0.8], intrinsics=K)
            plain.add(out, gt, [0.6, 0.8])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert ev.host_reads == 0 and len(ev) == 4
    assert ev.sources == ("network", "refined", "ransac", "select")
    names = tuple(f"{c}_{s}" for s in ev.sources for c in ("rot64", "trans64", "angle64")) + QUALITY + ("model",)
    assert ev.columns == COLUMNS + names and plain.columns == COLUMNS
    table = ev.rows(host=True).numpy()
    assert table[:, :len(COLUMNS)].tobytes() == plain.rows(host=True).numpy().tobytes()
    kw = {k: v for k, v in GEOMETRY.items()}
    for i, (out, gt, K) in enumerate(batches):
        found = mt.from_flows(out["flow"], K, out["rel_pose"], **kw)
        stack = torch.stack((out["rel_pose"], found["pose"], found["ransac"]["pose"], found["select"]["pose"]), dim=1).contiguous()
        errs = mt.pose_errors(stack, out["gt_rel_pose"]).cpu().numpy().reshape(2, 12)
        st = mt.residual_stats(found["matches"], K, torch.stack((out["gt_rel_pose"], out["rel_pose"]), dim=1).contiguous(), q=(0.5,),
                               thresholds=(1.0,))
        st = {k: v.cpu().numpy() for k, v in st.items()}
        with np.errstate(all="ignore"):
            share = st["within"][:, :, 0].astype(np.float64) / st["usable"].astype(np.float64)
        want = np.concatenate((errs, np.stack((found["matches"].count.cpu().numpy().astype(np.float64), st["usable"][:, 0].astype(np.float64),
                                               st["quant"][:, 0, 0], share[:, 0], st["sigma"][:, 0, 1], st["quant"][:, 1, 0], share[:, 1],
                                               found["select"]["model"].cpu().numpy().astype(np.float64)), axis=1)), axis=1)
        assert _same_bits(table[2 * i:2 * i + 2, len(COLUMNS):], want), (i, table[2 * i:2 * i + 2, len(COLUMNS):], want)
    c = {name: j for j, name in enumerate(ev.columns)}
    assert (table[:, c["matches"]] > 100).all() and (table[:, c["in_gt"]] > 0.9).all()           # exact flows: the truth fits
    assert (table[:, c["rot64_ransac"]] < np.radians(1.0)).all()                                  # and RANSAC finds it
    s = ev.summary()
    assert ev.host_reads == 2 and set(s) == {"all", "medium", "large"}
    base = plain.summary()
    for key, group in s.items():
        assert all(group[k] == v or (v != v and group[k] != group[k]) for k, v in base[key].items())      # the old keys, unchanged
        for src in ev.sources:
            for name in ("rot64", "angle64"):
                assert all(f"{name}_{src}_{stat}" in group for stat in ("mean", "median", "std"))
            assert all(0.0 <= group[f"auc{t}_{src}"] <= 1.0 for t in AUC_AT)
        assert all(name in group for name in QUALITY)
        assert abs(sum(group[f"model_{m}"] for m in ("E", "plane", "rotation", "none")) - 1.0) < 1e-12
    assert s["all"]["auc20_ransac"] > s["all"]["auc20_network"]          # half the network's poses are 30 degrees off
    text = ev.format_summary(s)
    assert len(text.splitlines()) == 3 * (1 + len(ev.sources)) and "all/ransac: Rot64_deg_mean: " in text and "AUC@20: " in text
    assert plain.format_summary(base) == "\n".join(l for l in text.splitlines() if "/" not in l.split(":")[0])
    with pytest.raises(ValueError, match="intrinsics"):
        ev.add(batches[0][0], batches[0][1], [0.6, 0.8])
    with pytest.raises(ValueError, match="unknown"):
        Evaluator(geometry={"ransack": {}})
    with pytest.raises(TypeError):
        plain.add(batches[0][0], batches[0][1], [0.6, 0.8], intrinsic=batches[0][2])
