"""coponerf_amd.triangulate.bundle_adjust on the MI355X (`pytest -m gpu`): cpn_bundle_adjust (csrc/bundle.hip, round 27 of the header)
against the restatement of tests/bundle_ref.py, pinned on the CPU by tests/test_bundle_ref.py, which also shows the margins that allow
the exact comparisons (no accept / reject, stop or depth decision of these fixtures within 1e-9 of its threshold).

bundle_ref.gpu_case(): B = 6, N = 768 - 600 noisy rows with outliers from refine_pose's result (some flags set), 257 rows (one more
than a workgroup) from a far start with accepted and rejected steps, 7 rows (below min_rows), 0 rows, a pose with t = 0, and pair 0
again under an inlier mask.  Every output starts as NaN between guards.
  iters = 0   only + - x / sqrt: every output in the BITS of the restatement.
  iters = 1, 10   a step takes the device library's sin and cos, so: the statuses, the rows used, the accepted and rejected counts,
              lambda, the first cost and the NaN pattern exactly; everything else within bundle_ref.output_bounds (the step bounds
              from operation counts, absolute sums and the measured cond(A) and cond(V), carried to every output by the rule's own
              derivatives, plus the last stage's rounding) and half an fp32 ulp for the fp32 stores.  The tests print error / bound.
The end-to-end tests on the synthetic weights only show that the paths run: those flows carry no geometry.
"""
import numpy as np
import pytest
import torch

from coponerf_amd import _hip
from tests import bundle_ref as br
from tests import matches_ref as mr
from tests.test_gpu_point_cloud import Guarded

pytestmark = pytest.mark.gpu

E_SHAPE, E_ARG = _hip.CONSTANTS["E_SHAPE"], _hip.CONSTANTS["E_ARG"]
SHAPES = {"pose": (4, 4), "xyz": (768, 3), "geom": (768, 4), "cov_x": (768, 6), "cov": (6, 6), "stats": (12,)}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want, dtype=got.dtype)
    bits = np.uint32 if got.dtype == np.float32 else np.uint64
    return bool(((got.view(bits) == want.view(bits)) | (np.isnan(got) & np.isnan(want))).all())


def _call(iters, dev, pairs=None):
    """cpn_bundle_adjust on gpu_case() (or on its pairs `pairs` alone), every output between guards -> (dict of arrays, their bytes)."""
    xy, counts, K, poses, xyz, flag, inlier = br.gpu_case()
    inlier = inlier.copy()
    inlier[:5] = 1                                                      # one mask for the batch: all ones but for pair 5
    sel = list(range(len(xy))) if pairs is None else list(pairs)
    B, N = len(sel), xy.shape[1]
    xd, cd, kd, pd, zd, fd, md = (_up(a[sel], dev) for a in (xy, counts, K, poses, xyz, flag, inlier))
    work = Guarded(B * 2 * N * 3, torch.float64, dev)
    out = {k: Guarded(B * int(np.prod(s)), torch.float64 if k in ("cov", "stats") else torch.float32, dev) for k, s in SHAPES.items()}
    _hip.call("cpn_bundle_adjust", xd.data_ptr(), cd.data_ptr(), kd.data_ptr(), pd.data_ptr(), zd.data_ptr(), fd.data_ptr(), md.data_ptr(),
              B, N, iters, br.GPU_SCALE, br.GPU_FTOL, 8, work.ptr, out["pose"].ptr, out["xyz"].ptr, out["geom"].ptr, out["cov_x"].ptr, out["cov"].ptr, out["stats"].ptr, _hip.stream_handle())
    work.get()
    got = {k: v.get().reshape((B,) + SHAPES[k]).copy() for k, v in out.items()}
    return got, b"".join(got[k].tobytes() for k in sorted(got))


def test_measuring_alone_in_bits(dev):
    """iters = 0: the costs, sigma, the pose's covariance and its two angles, the points, (z0, z1, e, w) and the points'
    covariances are the restatement's bits; status 2 for the pairs of 7 and 0 rows and for t = 0, with the pose as it came and
    NaN elsewhere; a second call gives the same bytes."""
    got, raw = _call(0, dev)
    want = br.want(0)
    poses = br.gpu_case()[3]
    for b, w in enumerate(want):
        for k in SHAPES:
            assert _same_bits(got[k][b], w[k]), (b, k)
    assert [int(v) for v in got["stats"][:, 11]] == [0, 0, 2, 2, 2, 0] and [int(v) for v in got["stats"][:, 3]] == [473, 257, 6, 0, 0, 320]
    for b in (2, 3, 4):
        assert got["pose"][b].tobytes() == poses[b].tobytes() and np.isnan(got["xyz"][b]).all() and np.isnan(got["cov"][b]).all()
    for b in (0, 1, 5):
        assert got["stats"][b, 0] == got["stats"][b, 1] and got["stats"][b, 4] == 0 and got["stats"][b, 10] == 0
        assert got["pose"][b, :3, :3].tobytes() == poses[b, :3, :3].tobytes()
    assert _call(0, dev)[1] == raw


@pytest.mark.parametrize("iters", [1, 10])
def test_steps_against_the_restatement(dev, iters):
    """The integers, lambda, the first cost and the NaN pattern exactly; every other figure within output_bounds plus the fp32
    store's half ulp; the kept cost never above the first; a pair alone gives the batch's bytes; a second call the same bytes.
    Observed on the MI355X (error / bound, the largest over the pairs): see the printed lines and DESIGN.md 4.25."""
    got, raw = _call(iters, dev)
    want = br.want(iters)
    for b, w in enumerate(want):
        exact = [3, 4, 5, 6, 11] + ([] if np.isnan(w["stats"][0]) else [0])
        assert _same_bits(got["stats"][b][exact], w["stats"][exact]), (b, got["stats"][b], w["stats"])
        for k in SHAPES:
            assert np.array_equal(np.isnan(got[k][b]), np.isnan(w[k])), (b, k)
        if w["stats"][11] == 2:
            assert _same_bits(got["pose"][b], w["pose"])
            continue
        bounds, steps = br.want_bounds(iters, b)
        assert got["stats"][b, 1] <= got["stats"][b, 0]
        for k64 in br.OUT64:
            k = br.STORED32.get(k64, k64)
            ref = w[k64]
            on = ~np.isnan(ref)
            bound = bounds[k64][on] + (mr.half_ulp32(ref[on]) if k64 in br.STORED32 else 0.0)
            err = np.abs(got[k][b].astype(np.float64)[on] - ref[on])
            ratio = float((err / np.maximum(bound, 1e-300)).max())
            print(f"iters {iters} pair {b} {k}: largest error / bound {ratio:.3g} (largest error {float(err.max()):.3g}); rounded-reference bits: "
                  f"{_same_bits(got[k][b], w[k])}")
            assert (err <= bound).all(), (b, k, ratio)
        print(f"iters {iters} pair {b}: step bounds {[f'{s[0]:.1e}' for s in steps]}, largest cond(A) {max(s[1] for s in steps):.3g}, "
              f"largest cond(V) {max(s[2] for s in steps):.3g}; accepted {int(w['stats'][4])}, rejected {int(w['stats'][5])}")
    assert [int(v) for v in got["stats"][:, 11]] == [0, 0, 2, 2, 2, 0]
    if iters == 10:
        assert got["stats"][1, 5] >= 1 and got["stats"][1, 4] >= 1     # steps of both kinds
    alone, _ = _call(iters, dev, pairs=(1,))
    assert all(alone[k][0].tobytes() == got[k][1].tobytes() for k in SHAPES)
    assert _call(iters, dev)[1] == raw


def test_wrapper_cloud_and_errors(dev):
    """triangulate.bundle_adjust returns the kernel's bytes; cloud's max_rel_sigma_z drops the rows its formula names and changes
    nothing without the keyword; the argument checks of the wrapper and the entry point's codes."""
    from coponerf_amd import matches as mt, triangulate as tg
    xy, counts, K, poses, xyz, flag, inlier = br.gpu_case()
    ref, _ = _call(10, dev, pairs=(0, 1, 2))
    sel = slice(0, 3)
    m = mt.Matches(_up(xy[sel], dev), torch.empty(3, 768, 2, device=dev), _up(counts[sel], dev))
    kd, pd = _up(K[sel], dev), _up(poses[sel], dev)
    tri = tg.points(m, kd, pd)
    assert tri["xyz"].cpu().numpy().tobytes() == xyz[sel].tobytes() and tri["flag"].cpu().numpy().tobytes() == flag[sel].tobytes()
    got = tg.bundle_adjust(tri, m, kd, pd, iters=10, scale_px=br.GPU_SCALE, ftol=br.GPU_FTOL)
    assert set(got) == set(SHAPES) and all(got[k].cpu().numpy().tobytes() == ref[k].tobytes() for k in SHAPES)
    masked = tg.bundle_adjust(tri, m, kd, pd, inlier=_up(inlier[5:6].repeat(3, 0), dev), iters=10, scale_px=br.GPU_SCALE, ftol=br.GPU_FTOL)
    assert masked["stats"][0, 3].item() == 320
    # the cloud: the adjusted points under the keep rule, then the relative depth sigma
    adj = {"xyz": got["xyz"], "geom": torch.cat((got["geom"][..., :3], tri["geom"][..., 3:]), -1), "flag": tri["flag"]}
    plain = tg.cloud(adj)
    sigma = got["stats"][:, 7]
    cut = tg.cloud(adj, max_rel_sigma_z=0.02, cov_x=got["cov_x"], sigma=sigma)
    g, c, f = adj["geom"].cpu().numpy(), got["cov_x"].cpu().numpy().astype(np.float64), flag[sel]
    with np.errstate(invalid="ignore"):
        keep = (f == 0) & (g[..., 2] <= np.float32(1.0)) & (g[..., 3] >= np.float32(1.0))
        small = sigma.cpu().numpy()[:, None] * np.sqrt(c[..., 5]) / g[..., 0].astype(np.float64) <= 0.02
    for b in range(2):
        assert len(plain.points(b)[0]) == int(keep[b].sum()) and len(cut.points(b)[0]) == int((keep[b] & small[b]).sum())
        assert 0 < int((keep[b] & small[b]).sum()) < int(keep[b].sum())
        assert cut.points(b)[0].tobytes() == got["xyz"][b].cpu().numpy()[keep[b] & small[b]].tobytes()
    for bad in (dict(iters=-1), dict(scale_px=0.0), dict(ftol=-1.0), dict(ftol=float("nan")), dict(min_rows=0)):
        with pytest.raises(ValueError):
            tg.bundle_adjust(tri, m, kd, pd, **bad)
    with pytest.raises(ValueError):
        tg.bundle_adjust({"xyz": tri["xyz"][:, :5].contiguous(), "flag": tri["flag"]}, m, kd, pd)
    with pytest.raises(ValueError):
        tg.bundle_adjust(tri, m, kd, pd, inlier=_up(inlier[:3, :5], dev))
    with pytest.raises(ValueError):
        tg.cloud(adj, max_rel_sigma_z=0.02)
    with pytest.raises(RuntimeError):
        tg.bundle_adjust(tri, m, kd, pd.cpu())
    fn = _hip.lib().cpn_bundle_adjust
    ok = (16, 16, 16, 16, 16, 16, None, 1, 8, 10, 1.0, 1e-12, 8, 16, 16, 16, 16, 16, 16, 16, None)
    swap = lambda i, v: ok[:i] + (v,) + ok[i + 1:]
    assert fn(*swap(7, 0)) == E_SHAPE and fn(*swap(8, 0)) == E_SHAPE and fn(*swap(7, 32768)) == E_SHAPE and fn(*swap(8, (1 << 24) + 1)) == E_SHAPE
    for i, v in ((0, None), (5, None), (13, None), (19, None), (9, -1), (10, 0.0), (10, float("inf")), (11, -1.0), (11, float("nan")), (12, 0)):
        assert fn(*swap(i, v)) == E_ARG, (i, v)


def test_from_flows_keyword(dev, monkeypatch):
    """Without triangulate['adjust'] from_flows makes the launches it made; with it one launch more and the key `adjust`: exact
    flows under RANSAC's pose adjust to a cost that is not above the first."""
    from coponerf_amd import matches as mt
    from tests import ransac_ref as rr
    f0, f1, K, Pt, _ = rr.flow_scene()
    flows, kd, pd = (_up(f0, dev), _up(f1, dev)), _up(K, dev), _up(Pt, dev)
    kw = dict(S=32, max_cycle_px=1e9, stride=2, ransac={"hypotheses": 64})
    calls = []
    real = _hip.call
    monkeypatch.setattr(_hip, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    before = mt.from_flows(flows, kd, pd, triangulate={"pose": "ransac"}, **kw)
    n_before = list(calls)
    del calls[:]
    after = mt.from_flows(flows, kd, pd, triangulate={"pose": "ransac", "adjust": {"iters": 5, "inliers_only": True}}, **kw)
    assert "adjust" not in before and calls == n_before + ["cpn_bundle_adjust"] and "cpn_bundle_adjust" not in n_before
    assert set(after) == set(before) | {"adjust"}
    assert after["points"]["xyz"].cpu().numpy().tobytes() == before["points"]["xyz"].cpu().numpy().tobytes()
    st = after["adjust"]["stats"][0].cpu().numpy()
    print("from_flows adjust stats", st)
    assert st[11] == 0 and st[1] <= st[0] and st[3] > 50
    for bad in ({"pose": "ransac", "adjust": {"passes": 3}}, {"pose": "ransac", "adjust": 5}, {"pose": "network", "adjust": {"inliers_only": True}}):
        with pytest.raises(ValueError):
            mt.from_flows(flows, kd, pd, triangulate=bad, **kw)


@pytest.fixture(scope="module")
def pair(dev):
    """The synthetic-weight model of the other GPU tests and one pair of 256 x 455 noise photos."""
    from coponerf_amd import CoPoNeRF, synthetic as syn
    from coponerf_amd.novel_views import prepare_pair
    model = CoPoNeRF.CoPoNeRF(n_view=2)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(syn.make_full_weights(shapes), strict=True)
    model = model.to(dev).eval()
    frames = syn.make_scene(n=2)[0]
    return model, prepare_pair(frames[0], frames[1], hfov_deg=75.0, device=dev)


def test_from_pair_and_evaluator_end_to_end(dev, pair, monkeypatch):
    """from_pair(adjust={}) and Evaluator(geometry={"triangulate": {.., "adjust": {}}}) on the synthetic weights: the paths run and
    return tensors of the stated shapes; without the keyword neither launches the kernel and Evaluator has no `adjusted` column.
    This shows that the paths run, nothing more."""
    from coponerf_amd import evaluate as ev, triangulate as tg
    model, inp = pair
    calls = []
    real = _hip.call
    monkeypatch.setattr(_hip, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    plain = tg.from_pair(model, inp, pose="refined", max_cycle_px=1e9)
    assert "adjust" not in plain and "cpn_bundle_adjust" not in calls
    res = tg.from_pair(model, inp, pose="refined", max_cycle_px=1e9, adjust={"iters": 3, "max_rel_sigma_z": 0.1})
    cap = 2 * 256 * 256
    ba = res["adjust"]
    assert calls.count("cpn_bundle_adjust") == 1 and tuple(ba["pose"].shape) == (1, 4, 4) and tuple(ba["cov_x"].shape) == (1, cap, 6)
    st = ba["stats"][0].cpu().numpy()
    xyz, _ = res["cloud"].points(0)
    print("from_pair adjust stats", st, "; cloud", len(xyz))
    assert st[11] in (0.0, 1.0, 2.0) and np.isfinite(ba["pose"].cpu().numpy()).all() and len(xyz) <= int(res["matches"]["matches"].count[0])
    with pytest.raises(ValueError):
        tg.from_pair(model, inp, adjust={"passes": 1})
    assert "adjusted" in ev.SOURCES
    without = ev.Evaluator(geometry={"max_cycle_px": 1e9})
    with_it = ev.Evaluator(geometry={"max_cycle_px": 1e9, "triangulate": {"pose": "refined", "adjust": {"iters": 3}}})
    assert "adjusted" not in without.sources and not any(c.endswith("_adjusted") for c in without.columns)
    assert with_it.sources[-1] == "adjusted" and {"rot64_adjusted", "trans64_adjusted", "angle64_adjusted"} <= set(with_it.columns)
    assert [c for c in with_it.columns if not c.endswith("_adjusted")] == list(without.columns)
    with pytest.raises(ValueError):
        ev.Evaluator(geometry={"triangulate": {"pose": "refined"}})
    del calls[:]
    found = pair[0].get_z(inp)
    out = {"flow": found[2], "rel_pose": found[1]}
    rel, K = found[1].float().contiguous(), inp["context"]["intrinsics"].float().contiguous()
    for e in (without, with_it):
        e._reserve(1, dev)
        rows = torch.full((1, len(e.columns)), float("nan"), dtype=torch.float64, device=dev)
        e._add_geometry(rows, out["flow"], rel, rel, K)
        if e is without:
            assert "cpn_bundle_adjust" not in calls
            base = rows.cpu().numpy()
        else:
            assert calls.count("cpn_bundle_adjust") == 1
            cols = [i for i, c in enumerate(e.columns) if not c.endswith("_adjusted")]
            assert rows.cpu().numpy()[:, cols].tobytes() == base.tobytes()     # the existing columns keep their bytes
