"""coponerf_amd.triangulate on the MI355X (`pytest -m gpu`): cpn_triangulate_matches and cpn_depth_scale (csrc/triangulate.hip, round
26 of the header) against the restatement of tests/triangulate_ref.py, pinned on the CPU by tests/test_triangulate_ref.py, which also
shows the margins that allow the exact comparisons.

cpn_triangulate_matches: triangulate_ref.scene_case() - B = 2, N = 768, counts 257 and 511: more rows than a workgroup, no multiple of
256, NaN beyond the counts, two photos for the colours - and constructed_case(): an exact match (c = 0), a match on both epipoles, a
zero-parallax row, a point behind one camera (each in turn, by the sign of t), one behind both, a NaN row inside the count and a 176 px
outlier.  Every output starts as NaN / 255 between guards.  The flags exactly; xyz, z0, z1, the error and the colours in the BITS of
the restatement rounded to fp32; the parallax within 1 fp32 ulp (it takes the device library's atan2); a second call the same bytes.
cpn_depth_scale: scale_case() - counts 768, 0, 1, 7 and 8, either side of min_rows = 8, and a pose of zero translation: the rows used
exactly, the scale, the spread and the ratio in their bits.
The end-to-end test on the synthetic weights only shows that the path runs: those flows carry no geometry.
"""
import numpy as np
import pytest
import torch

from coponerf_amd import _hip
from tests import ransac_ref as rr
from tests import triangulate_ref as tr
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


def _same_bits(got, want):
    """Equal as bit patterns (so +0 is not -0), every NaN equal to every NaN; fp32 or float64."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want, dtype=got.dtype)
    bits = np.uint32 if got.dtype == np.float32 else np.uint64
    return bool(((got.view(bits) == want.view(bits)) | (np.isnan(got) & np.isnan(want))).all())


def _points_call(case, dev):
    """cpn_triangulate_matches on a fixture of triangulate_ref, every output between guards -> dict of arrays and their bytes."""
    if case == "scene":
        xy, counts, K, poses, images = tr.scene_case()
    else:
        (xy, counts, K, poses), images = tr.constructed_case(), None
    B, N = xy.shape[:2]
    xd, cd, kd, pd = _up(xy, dev), _up(counts, dev), _up(K, dev), _up(poses, dev)
    im = _up(images, dev) if images is not None else None
    out = {"xyz": Guarded(B * N * 3, torch.float32, dev), "geom": Guarded(B * N * 4, torch.float32, dev),
           "flag": Guarded(B * N, torch.uint8, dev)}
    if im is not None:
        out["rgb"] = Guarded(B * N * 3, torch.float32, dev)
    _hip.call("cpn_triangulate_matches", xd.data_ptr(), cd.data_ptr(), kd.data_ptr(), pd.data_ptr(), im.data_ptr() if im is not None else None,
              B, N, int(images.shape[2]) if images is not None else 0, out["xyz"].ptr, out["geom"].ptr, out["flag"].ptr,
              out["rgb"].ptr if im is not None else None, _hip.stream_handle())
    shapes = {"xyz": (B, N, 3), "geom": (B, N, 4), "flag": (B, N), "rgb": (B, N, 3)}
    got = {k: v.get().reshape(shapes[k]).copy() for k, v in out.items()}
    return got, b"".join(got[k].tobytes() for k in sorted(got))


@pytest.mark.parametrize("case", ["scene", "constructed"])
def test_points_against_the_restatement(dev, case):
    """The flags exactly; xyz, z0, z1, the error and the colours in their bits; the parallax within 1 fp32 ulp; NaN and 255 at and
    beyond the counts; the guards hold; a second call gives the same bytes.  Largest parallax difference on gfx950: the printed figure."""
    got, raw = _points_call(case, dev)
    want = tr.want_points(case)
    counts = (tr.scene_case() if case == "scene" else tr.constructed_case())[1]
    worst = 0.0
    for b, w in enumerate(want):
        assert np.array_equal(got["flag"][b], w["flag"]), (case, b, np.flatnonzero(got["flag"][b] != w["flag"]))
        assert _same_bits(got["xyz"][b], w["xyz"]), (case, b)
        assert _same_bits(got["geom"][b][:, :3], w["geom"][:, :3]), (case, b)
        if "rgb" in w:
            assert _same_bits(got["rgb"][b], w["rgb"]), (case, b)
        par, ref = got["geom"][b][:, 3], w["geom"][:, 3]
        assert np.array_equal(np.isnan(par), np.isnan(ref))
        on = ~np.isnan(ref)
        ulp = np.abs(par[on].astype(np.float64) - ref[on].astype(np.float64)) / np.spacing(np.maximum(np.abs(ref[on]), np.float32(1e-30))).astype(np.float64)
        worst = max(worst, float(ulp.max()))
        assert (got["flag"][b][counts[b]:] == 255).all() and np.isnan(got["xyz"][b][counts[b]:]).all() and np.isnan(got["geom"][b][counts[b]:]).all()
    print(f"cpn_triangulate_matches ({case}): largest parallax difference {worst:.2f} fp32 ulp")
    assert worst <= 1.0
    assert _points_call(case, dev)[1] == raw                             # determinism
    if case == "constructed":
        I, C, P, B0, B1 = tr.INPUT, tr.CORRECTION, tr.PARALLAX, tr.BEHIND0, tr.BEHIND1
        assert [int(v) for v in got["flag"][0][:7]] == [0, C | P | B0 | B1, P | B0 | B1, B1, B0 | B1, I, 0]
        assert [int(v) for v in got["flag"][1][:7]] == [0, C | P | B0 | B1, P | B0 | B1, B0, B0 | B1, I, B0 | B1]
        assert got["geom"][0][0].tolist()[:3] == [2.0, 1.0, 0.0] and got["xyz"][0][0].tolist() == [0.25, 0.5, 2.0]      # the exact match
        assert 30.0 < got["geom"][0][6][2] < 176.0                      # the outlier is moved back onto the constraint
    else:
        assert {int(v) for v in got["flag"].reshape(-1)} == {0, tr.BEHIND0 | tr.BEHIND1, 255}


def _scale_call(dev):
    geom, flag, xy, counts, depth, rel = tr.scale_case()
    B, N = flag.shape
    scale, stats = Guarded(B, torch.float64, dev), Guarded(B * 4, torch.float64, dev)
    gd, fd, xd, cd, dd, rd = (_up(a, dev) for a in (geom, flag, xy, counts, depth, rel))
    _hip.call("cpn_depth_scale", gd.data_ptr(), fd.data_ptr(), xd.data_ptr(), cd.data_ptr(), dd.data_ptr(), rd.data_ptr(), B, N, tr.S_GPU,
              1.0, 1.0, 8, scale.ptr, stats.ptr, _hip.stream_handle())
    return scale.get().copy(), stats.get().reshape(B, 4).copy()


def test_depth_scale_against_the_restatement(dev):
    """Counts 768, 0, 1, 7, 8 and a pose without a translation: the rows used and the status exactly, the scale, the spread and the
    ratio in their bits (a division and a square root are exact); a second call gives the same bytes."""
    scale, stats = _scale_call(dev)
    want = tr.want_scales()
    for b, (s, st) in enumerate(want):
        assert stats[b, 0] == st[0] and stats[b, 3] == st[3], (b, stats[b], st)
        assert _same_bits(scale[b:b + 1], np.array([s])), (b, scale[b], s)
        assert _same_bits(stats[b], st), (b, stats[b], st)
    assert [int(v) for v in stats[:, 0]] == [529, 0, 1, 7, 8, 0] and [int(v) for v in stats[:, 3]] == [0, 1, 1, 1, 0, 1]
    again = _scale_call(dev)
    assert again[0].tobytes() == scale.tobytes() and again[1].tobytes() == stats.tobytes()
    geom, flag, xy, counts, depth, rel = (_up(a, dev) for a in tr.scale_case())
    none = Guarded(6 * 4, torch.float64, dev)
    sc = Guarded(6, torch.float64, dev)
    _hip.call("cpn_depth_scale", geom.data_ptr(), flag.data_ptr(), xy.data_ptr(), counts.data_ptr(), depth.data_ptr(), None, 6, 768, tr.S_GPU,
              1.0, 1.0, 8, sc.ptr, none.ptr, _hip.stream_handle())
    assert np.isnan(none.get().reshape(6, 4)[:, 2]).all() and sc.get().tobytes() == scale.tobytes()      # no rel_pose: the ratio is NaN


def test_wrappers_cloud_and_errors(dev):
    """triangulate.points, depth_scale, rescale and cloud: the kernels' bytes; the cloud has the rows, the order and the colours of
    the restatement's keep mask (with and without an inlier mask); the checks of the arguments and the entry points' codes."""
    from coponerf_amd import matches as mt, triangulate as tg
    xy, counts, K, poses, images = tr.scene_case()
    m = mt.Matches(_up(xy, dev), torch.empty(2, 768, 2, device=dev), _up(counts, dev))
    kd, pd, im = _up(K, dev), _up(poses, dev), _up(images, dev)
    ref, _ = _points_call("scene", dev)
    got = tg.points(m, kd, pd, im)
    assert set(got) == {"xyz", "geom", "flag", "rgb"} and all(got[k].cpu().numpy().tobytes() == ref[k].tobytes() for k in ref)
    plain = tg.points(m, kd, pd)
    assert set(plain) == {"xyz", "geom", "flag"} and plain["xyz"].cpu().numpy().tobytes() == ref["xyz"].tobytes()
    inlier = (np.arange(768)[None, :] % 3 != 0).astype(np.uint8).repeat(2, 0)
    want = tr.want_points("scene")
    for mask in (None, inlier):
        pc = tg.cloud(got, inlier=None if mask is None else _up(mask, dev))
        grey = tg.cloud(plain, inlier=None if mask is None else _up(mask, dev))
        for b in range(2):
            xyz, rgb = pc.points(b)
            wx, wc = tr.cloud(want[b], inlier=None if mask is None else mask[b])
            assert len(wx) > 50 and xyz.tobytes() == wx.tobytes() and rgb.tobytes() == wc.tobytes(), (b, len(xyz), len(wx))
            gx, gc = grey.points(b)
            assert gx.tobytes() == wx.tobytes() and (gc == 127).all() | (gc == 128).all()
    # rescale: [R | s t / |t|], a NaN scale keeps the pose
    s = torch.tensor([2.5, float("nan")], dtype=torch.float64, device=dev)
    moved = tg.rescale(pd, s).cpu().numpy()
    t0 = poses[0, :3, 3].astype(np.float64)
    assert moved[0, :3, 3].tobytes() == (2.5 * (t0 / np.linalg.norm(t0))).astype(np.float32).tobytes()
    assert moved[1].tobytes() == poses[1].tobytes() and moved[0, :3, :3].tobytes() == poses[0, :3, :3].tobytes()
    # depth_scale's wrapper
    geom, flag, sxy, scounts, depth, rel = (_up(a, dev) for a in tr.scale_case())
    sm = mt.Matches(sxy, torch.empty(6, 768, 2, device=dev), scounts)
    ds = tg.depth_scale({"geom": geom, "flag": flag}, sm, depth, tr.S_GPU, rel_pose=rel)
    scale, stats = _scale_call(dev)
    assert ds["scale"].cpu().numpy().tobytes() == scale.tobytes() and ds["stats"].cpu().numpy().tobytes() == stats.tobytes()
    for bad in (dict(S=255), dict(min_rows=0), dict(max_reproj_px=-1.0), dict(min_parallax_deg=float("nan"))):
        with pytest.raises(ValueError):
            tg.depth_scale({"geom": geom, "flag": flag}, sm, depth, **{"S": tr.S_GPU, **bad})
    with pytest.raises(ValueError):
        tg.points(m, kd, pd, im[:, :1].contiguous())
    with pytest.raises(ValueError):
        tg.points(m, kd, pd[:1].contiguous())
    with pytest.raises(RuntimeError):
        tg.points(m, kd, pd.cpu())
    with pytest.raises(ValueError):
        tg.cloud(got, inlier=_up(inlier[:, :5], dev))
    fn, gn = _hip.lib().cpn_triangulate_matches, _hip.lib().cpn_depth_scale
    assert fn(16, 16, 16, 16, None, 0, 8, 0, 16, 16, 16, None, None) == E_SHAPE and fn(16, 16, 16, 16, None, 1, 0, 0, 16, 16, 16, None, None) == E_SHAPE
    assert fn(16, 16, 16, 16, 16, 1, 8, 0, 16, 16, 16, 16, None) == E_SHAPE
    assert fn(16, 16, 16, 16, 16, 1, 8, 4, 16, 16, 16, None, None) == E_ARG and fn(16, None, 16, 16, None, 1, 8, 0, 16, 16, 16, None, None) == E_ARG
    assert gn(16, 16, 16, 16, 16, None, 1, 8, 0, 1.0, 1.0, 8, 16, 16, None) == E_SHAPE
    assert gn(16, 16, 16, 16, 16, None, 1, 8, 4, 1.0, 1.0, 0, 16, 16, None) == E_ARG
    assert gn(16, 16, 16, 16, 16, None, 1, 8, 4, -1.0, 1.0, 8, 16, 16, None) == E_ARG
    assert gn(16, 16, 16, 16, None, None, 1, 8, 4, 1.0, 1.0, 8, 16, 16, None) == E_ARG


def test_from_flows_keyword(dev, monkeypatch):
    """Without triangulate= from_flows makes the launches it made and returns the same bytes; with it, one launch more and the key
    `points`: exact flows under the true pose triangulate in front of both cameras."""
    from coponerf_amd import matches as mt
    f0, f1, K, Pt, _ = rr.flow_scene()
    flows, kd, pd = (_up(f0, dev), _up(f1, dev)), _up(K, dev), _up(Pt, dev)
    kw = dict(S=32, max_cycle_px=1e9, stride=2, ransac={"hypotheses": 64})
    calls = []
    real = _hip.call
    monkeypatch.setattr(_hip, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    before = mt.from_flows(flows, kd, pd, **kw)
    n_before = list(calls)
    del calls[:]
    after = mt.from_flows(flows, kd, pd, triangulate={"pose": "ransac"}, **kw)
    assert "points" not in before and calls == n_before + ["cpn_triangulate_matches"] and "cpn_triangulate_matches" not in n_before
    assert set(after) == set(before) | {"points"}
    for key in ("pose", "stats", "rel_pose"):
        assert after[key].cpu().numpy().tobytes() == before[key].cpu().numpy().tobytes(), key
    n = int(after["matches"].count[0])
    assert n == int(before["matches"].count[0])
    for key in ("xy", "err"):                                            # the rows beyond the count are not written
        assert getattr(after["matches"], key)[0, :n].cpu().numpy().tobytes() == getattr(before["matches"], key)[0, :n].cpu().numpy().tobytes(), key
    for k in ("pose", "stats"):
        assert after["ransac"][k].cpu().numpy().tobytes() == before["ransac"][k].cpu().numpy().tobytes(), k
    assert after["ransac"]["inlier"][0, :n].cpu().numpy().tobytes() == before["ransac"]["inlier"][0, :n].cpu().numpy().tobytes()
    flag = after["points"]["flag"][0].cpu().numpy()
    assert n > 100 and (flag[:n] == 0).mean() > 0.9 and (flag[n:] == 255).all()
    for bad in ({"pose": "selected"}, {"pose": "refined", "depth": 1}, {"pose": "best"}, "ransac"):
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


def test_from_pair_end_to_end(dev, pair):
    """from_pair with scale="depth" on the synthetic weights: the path runs - matches, points under |t| = 1, one render of view 0's
    depth, depth_scale, rescale, points, cloud - and returns tensors of the stated shapes; the cloud is empty or tiny, because these
    flows carry no geometry.  This shows that the path runs, nothing more."""
    from coponerf_amd import triangulate as tg
    model, inp = pair
    res = tg.from_pair(model, inp, pose="network", scale="depth", max_cycle_px=1e9)
    cap = 2 * 256 * 256
    assert tuple(res["pose"].shape) == (1, 4, 4) and tuple(res["scale"].shape) == (1,) and tuple(res["stats"].shape) == (1, 4)
    assert tuple(res["points"]["xyz"].shape) == (1, cap, 3) and tuple(res["points"]["rgb"].shape) == (1, cap, 3)
    stats = res["stats"][0].cpu().numpy()
    xyz, rgb = res["cloud"].points(0)
    n = int(res["matches"]["matches"].count[0])
    print("matches", n, "; depth_scale stats", stats, "; scale", float(res["scale"][0]), "; cloud", len(xyz))
    assert stats[3] in (0.0, 1.0) and 0 <= stats[0] <= n and len(xyz) <= n and xyz.shape == (len(xyz), 3) and rgb.dtype == np.uint8
    assert np.isfinite(res["pose"].cpu().numpy()).all()
    if stats[3] == 1.0:                                                  # too few rows: the pose keeps the network's length
        assert torch.equal(res["pose"], res["matches"]["rel_pose"])
    given = tg.from_pair(model, inp, pose="selected", scale="given", max_cycle_px=1e9, select={"hypotheses": 64})
    assert given["scale"] is None and given["stats"] is None and torch.equal(given["pose"], given["matches"]["select"]["pose"])
    with pytest.raises(ValueError):
        tg.from_pair(model, inp, pose="best")
    with pytest.raises(ValueError):
        tg.from_pair(model, inp, scale="median")
