"""coponerf_amd.point_cloud on the MI355X (`pytest -m gpu`): the kernels of csrc/point_cloud.hip element by element against the
float64 restatements of tests/point_cloud_ref.py (pinned on the CPU by tests/test_point_cloud_ref.py), and reconstruct end to end.

Every output buffer starts as NaN (floats) or 0xFF (bytes, counts) between guard rows; nothing is left out of a comparison
except the pixels with a decision inside the 1e-9 band of a threshold, which are counted and held to 1e-3 of all pixels.
Bounds (tests/point_cloud_ref.py, from operation counts): points and depth_fused half an fp32 ulp of the result plus
8 (51 + K for the round trip) 2^-53 times the sum of the absolute terms; votes, counts and compacted bytes exactly.
"""
import warnings

import numpy as np
import pytest
import torch

from coponerf_amd import _hip, synthetic as syn
from tests import point_cloud_ref as pr
from tests.test_point_cloud_ref import _parse_ply

pytestmark = pytest.mark.gpu

GUARD = 64                                                    # elements in front of and behind every output


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


class Guarded:
    """An output of n elements between two guards, all filled with `fill` (NaN or 0xFF bytes)."""

    def __init__(self, n, dtype, dev):
        self.n, self.fill = n, float("nan") if dtype.is_floating_point else (255 if dtype == torch.uint8 else -1)
        self.all = torch.full((n + 2 * GUARD,), self.fill, dtype=dtype, device=dev)
        self.ptr = self.all.data_ptr() + GUARD * self.all.element_size()

    def get(self):
        a = self.all.cpu().numpy()
        for g in (a[:GUARD], a[GUARD + self.n:]):
            assert np.isnan(g).all() if np.isnan(self.fill) else (g == self.fill).all(), "guard overwritten"
        return a[GUARD:GUARD + self.n]


def _upload(case, dev):
    return tuple(torch.from_numpy(np.array(case[k])).to(dev) for k in ("depth", "poses", "intrinsics"))


def _run_points(case, dev):
    depth, poses, intr = _upload(case, dev)
    K, B, R = depth.shape
    y0, x0, h, w = pr.window_of(case["S"], case["window"])
    xyz = Guarded(K * B * R * 3, torch.float32, dev)
    _hip.call("cpn_depth_points", depth.data_ptr(), poses.data_ptr(), intr.data_ptr(), K, B, case["S"], y0, x0, h, w, xyz.ptr,
              _hip.stream_handle())
    return xyz.get().reshape(K, B, R, 3)


def _run_votes(case, dev):
    depth, poses, intr = _upload(case, dev)
    K, B, R = depth.shape
    y0, x0, h, w = pr.window_of(case["S"], case["window"])
    votes, fused = Guarded(K * B * R, torch.uint8, dev), Guarded(K * B * R, torch.float32, dev)
    _hip.call("cpn_depth_votes", depth.data_ptr(), poses.data_ptr(), intr.data_ptr(), K, B, case["S"], y0, x0, h, w, pr.PX_TOL,
              pr.REL_TOL, votes.ptr, fused.ptr, _hip.stream_handle())
    return votes.get().reshape(K, B, R), fused.get().reshape(K, B, R)


CASES = ["main", "K1", "K2", "whole"]


# ----------------------------------------------------------------------------------------------------------------- points
@pytest.mark.parametrize("name", CASES)
def test_depth_points_against_float64(dev, name):
    case = pr.all_cases()[name]
    ref, bound = pr.depth_points(case["depth"], case["poses"], case["intrinsics"], case["S"], case["window"])
    got = _run_points(case, dev).astype(np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(ref))         # NaN exactly where the depth is not valid
    ok = ~np.isnan(ref)
    err = np.abs(got - ref)[ok]
    print(name, "points: largest error / bound", float((err / bound[ok]).max()), "of", int(ok.sum()), "components")
    assert ok.sum() > 0.9 * ref.size and (err <= bound[ok]).all()


# ------------------------------------------------------------------------------------------------------------------ votes
@pytest.mark.parametrize("name", CASES)
def test_depth_votes_against_float64(dev, name):
    case = pr.all_cases()[name]
    ref = pr.votes_of(case)
    votes, fused = _run_votes(case, dev)
    in_band = ref["near"].any(axis=1)                            # (K, B, R): a decision of the pixel near its threshold
    print(name, "pixels in the band", int(in_band.sum()), "of", in_band.size)
    assert in_band.sum() <= pr.BAND_SHARE * in_band.size
    assert np.array_equal(votes[~in_band], ref["votes"][~in_band])
    assert np.array_equal(np.isnan(fused), np.isnan(ref["fused"]))               # NaN exactly where d_a is not valid
    agree = (votes == ref["votes"]) & ~np.isnan(ref["fused"])
    err = np.abs(fused.astype(np.float64) - ref["fused"])[agree]
    print(name, "depth_fused: largest error / bound", float((err / ref["fused_bound"][agree]).max()), "of", int(agree.sum()))
    assert (err <= ref["fused_bound"][agree]).all()
    if name == "K1":
        assert not votes.any()


def test_bad_shapes_are_status_codes(dev):
    """K = 0, K = 256 and h = 0 come back as CPN_E_SHAPE before any launch (the pointers are one small valid buffer)."""
    lib = _hip.lib()
    buf = torch.zeros(4096, dtype=torch.float32, device=dev)
    p, s = buf.data_ptr(), _hip.stream_handle()
    for K, h in ((0, 4), (256, 4), (2, 0)):
        assert lib.cpn_depth_points(p, p, p, K, 1, 8, 0, 0, h, 4, p, s) == _hip.CONSTANTS["E_SHAPE"]
        assert b"cpn_depth_points" in lib.cpn_last_error()
        assert lib.cpn_depth_votes(p, p, p, K, 1, 8, 0, 0, h, 4, 1.0, 0.01, p, p, s) == _hip.CONSTANTS["E_SHAPE"]
        assert lib.cpn_compact_points(p, p, p, K, 1, h, 4, p, p, p, p, s) == _hip.CONSTANTS["E_SHAPE"]
        assert lib.cpn_compact_points_scratch(K, 1, h, 4) == 0
    assert lib.cpn_depth_points(p, p, p, 2, 1, 8, 6, 0, 4, 4, p, s) == _hip.CONSTANTS["E_SHAPE"]      # the window leaves the grid
    torch.cuda.synchronize()
    assert not bool(buf.any())                                   # nothing ran


# ------------------------------------------------------------------------------------------------------------- compaction
def _run_compact(keep, xyz, rgb, h, w, dev):
    K, B, R = keep.shape
    cap = K * R
    kd, xd, cd = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (keep, xyz, rgb))
    n_scratch = _hip.lib().cpn_compact_points_scratch(K, B, h, w)
    assert n_scratch == B * -(-cap // _hip.CONSTANTS["COMPACT_TILE"])
    scratch = torch.empty(n_scratch, dtype=torch.int32, device=dev)
    oxyz, orgb, count = Guarded(B * cap * 3, torch.float32, dev), Guarded(B * cap * 3, torch.uint8, dev), Guarded(B, torch.int32, dev)
    _hip.call("cpn_compact_points", kd.data_ptr(), xd.data_ptr(), cd.data_ptr(), K, B, h, w, scratch.data_ptr(), oxyz.ptr, orgb.ptr,
              count.ptr, _hip.stream_handle())
    return oxyz.get().reshape(B, cap, 3), orgb.get().reshape(B, cap, 3), count.get()


def _check_compact(keep, xyz, rgb, h, w, dev):
    want_xyz, want_rgb, want_n = pr.compact(keep, xyz, rgb)
    got = _run_compact(keep, xyz, rgb, h, w, dev)
    assert np.array_equal(got[2], want_n)
    for b in range(keep.shape[1]):
        n = int(want_n[b])
        assert got[0][b, :n].tobytes() == want_xyz[b].tobytes() and got[1][b, :n].tobytes() == want_rgb[b].tobytes()
        assert np.isnan(got[0][b, n:]).all() and (got[1][b, n:] == 255).all()      # rows beyond the count: untouched
    again = _run_compact(keep, xyz, rgb, h, w, dev)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))               # two runs, the same bytes
    return want_n


def test_compact_main_case_and_the_two_ends(dev):
    case = pr.main_case()
    K, B, R = case["depth"].shape
    xyz = _run_points(case, dev)                                  # with its NaN rows: the kernel copies bits
    rgb = pr.colours((K, B, R, 3))
    keep = (pr.valid(case["depth"]) & (pr.votes_of(case)["votes"] >= 1)).astype(np.uint8) * 3
    n = _check_compact(keep, xyz, rgb, case["h"], case["w"], dev)
    assert (n > 0.2 * K * R).all() and (n < 0.8 * K * R).all()
    assert (_check_compact(np.ones_like(keep), xyz, rgb, case["h"], case["w"], dev) == K * R).all()
    assert (_check_compact(np.zeros_like(keep), xyz, rgb, case["h"], case["w"], dev) == 0).all()


def test_compact_more_blocks_than_one_pass_of_the_finish(dev):
    """2^20 elements of one pair are 2^20 / CPN_COMPACT_TILE = 1 024 workgroups; the finishing step - the sum of the counts of
    the workgroups before one's own - covers CPN_COMPACT_FINISH = 256 counts per pass, so the last workgroups walk four."""
    tile, width = _hip.CONSTANTS["COMPACT_TILE"], _hip.CONSTANTS["COMPACT_FINISH"]
    K, h, w = 4, 512, 512
    assert (tile, width) == (1024, 256) and K * h * w == 2 ** 20 and K * h * w // tile > width
    rng = np.random.default_rng(15)
    keep = (rng.random((K, 1, h * w)) < 0.37).astype(np.uint8)
    keep[1, 0, 1000:200000] = 0                                   # long runs of empty and of full workgroups
    keep[2, 0, 5000:90000] = 1
    xyz = rng.normal(size=(K, 1, h * w, 3)).astype(np.float32)
    n = _check_compact(keep, xyz, pr.colours((K, 1, h * w, 3)), h, w, dev)
    assert 0.2 * 2 ** 20 < n[0] < 0.8 * 2 ** 20


# ------------------------------------------------------------------------------------------------------------- end to end
WINDOW = (100, 37, 32, 48)
TS = (0.0, 1.0)


@pytest.fixture(scope="module")
def scene(dev):
    """The synthetic-weight model of the other GPU tests, one pair of 256 x 455 noise photos, and its two views with depth."""
    from coponerf_amd import CoPoNeRF
    from coponerf_amd.novel_views import prepare_pair, render_path
    model = CoPoNeRF.CoPoNeRF(n_view=2)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(syn.make_full_weights(shapes), strict=True)
    model = model.to(dev).eval()
    frames = syn.make_scene(n=2)[0]
    inp = prepare_pair(frames[0], frames[1], hfov_deg=75.0, device=dev)
    views = render_path(model, inp, TS, window=WINDOW, return_rgb=True, return_depth=True)
    return model, inp, views


def _plain(model, inp, pose, uv, latents):
    z, rel_pose, flow = latents
    B, R = uv.shape[0], uv.shape[2]
    query = {"uv": uv, "rgb": torch.zeros(B, 1, R, 3, device=uv.device), "intrinsics": inp["query"]["intrinsics"],
             "cam2world": pose.unsqueeze(1).contiguous()}
    with torch.no_grad():
        return model({"context": inp["context"], "query": query}, z=z, rel_pose=rel_pose, val=True, flow=flow)


def _window_uv(inp):
    y0, x0, h, w = WINDOW
    return inp["query"]["uv"].view(1, 1, 256, 256, 2)[:, :, y0:y0 + h, x0:x0 + w].reshape(1, 1, h * w, 2).contiguous()


def test_render_path_hands_depth_over(dev, scene):
    from coponerf_amd.novel_views import render_path
    model, inp, views = scene
    y0, x0, h, w = WINDOW
    assert set(render_path(model, inp, TS, window=WINDOW)) == {"frames", "poses", "rel_pose"}          # as before
    assert set(views) == {"frames", "poses", "rel_pose", "rgb", "depth", "valid"}
    assert views["depth"].shape == (2, 1, h * w) and views["depth"].dtype == torch.float32
    assert views["valid"].shape == (2, 1, h * w) and views["valid"].dtype == torch.uint8
    with torch.no_grad():
        latents = model.get_z(inp)
    for k in range(2):
        plain = _plain(model, inp, views["poses"][k], _window_uv(inp), latents)
        assert torch.equal(views["rgb"][k], plain["rgb"].view(1, h * w, 3)), k
        assert torch.equal(views["depth"][k], plain["depth_ray"].view(1, h * w)), k
        assert torch.equal(views["valid"][k] != 0, plain["valid_mask"].view(1, h * w) != 0), k


def test_points_agree_with_forwards_own_reprojection(dev, scene):
    """View t = 0 is context view 0's own camera, so forward's `T_to_C1_pts` is the pixel each point of that view falls on in
    context view 0.  That output is fp32 (csrc/rayout.hip: reproject): K^-1 (u, v, 1) scaled by the depth (5 operations on two
    rounded entries of the inverse), the rigid transform (6, exact for the identity), two homogeneous divisions by w + 1e-6
    (4) and K (4): about twenty operations on terms of size |u| + 2 |cx| in pixels - 20 U (|u| + 2 |cx|), to which the two
    fp32 roundings of the point compared (x or y, and z) add 2 U.  The same formula in float64 on cpn_depth_points' points
    must land within that; the bound rests on the existing output's arithmetic, not on the new kernel's."""
    from coponerf_amd.point_cloud import unproject
    model, inp, views = scene
    y0, x0, h, w = WINDOW
    with torch.no_grad():
        latents = model.get_z(inp)
    plain = _plain(model, inp, views["poses"][0], _window_uv(inp), latents)
    assert torch.equal(views["poses"][0, 0], torch.eye(4, device=dev))
    xyz = unproject(views["depth"][:1], views["poses"][:1], inp["query"]["intrinsics"], 256, window=WINDOW)[0, 0].cpu().numpy()
    ok = pr.valid(views["depth"][0, 0].cpu().numpy())
    print("valid depths of view 0:", int(ok.sum()), "of", ok.size)
    assert ok.sum() >= 0.05 * ok.size                            # the statement is about something
    assert np.array_equal(np.isnan(xyz).any(axis=1), ~ok)
    K0 = inp["context"]["intrinsics"][0, 0].cpu().numpy().astype(np.float64)
    eps = float(np.float32(1e-6))
    c = xyz[ok].astype(np.float64) / (1.0 + eps)
    rr = c @ K0[:3, :3].T
    want = rr[:, :2] / (rr[:, 2:] + eps)
    got = plain["T_to_C1_pts"][0].cpu().numpy().astype(np.float64)[ok]
    uv = _window_uv(inp)[0, 0].cpu().numpy().astype(np.float64)[ok]
    bound = 22 * pr.U * (np.abs(uv) + 2 * np.abs(K0[:2, 2]))
    print("reprojection: largest error / bound", float((np.abs(got - want) / bound).max()))
    assert (np.abs(got - want) <= bound).all()


def _defaults_against_float64(model, inp, ts, dev):
    """reconstruct with its defaults on the views at ts: the votes behind it are the float64 reference's outside the band, and
    the cloud - made under sync-debug "error" - is exactly the selection they make.  Returns the cloud and its host arrays."""
    from coponerf_amd import point_cloud as pc
    from coponerf_amd.novel_views import render_path
    Kq = inp["query"]["intrinsics"]
    views = render_path(model, inp, ts, window=WINDOW, return_rgb=True, return_depth=True)
    depth, seen = views["depth"].cpu().numpy(), views["valid"].cpu().numpy() != 0
    votes, fused = pc.vote(views["depth"], views["poses"], Kq, 256, 1.0, 0.01, window=WINDOW)
    ref = pr.depth_votes(depth, views["poses"].cpu().numpy(), Kq[:, 0].cpu().numpy(), 256, window=WINDOW)
    in_band = ref["near"].any(axis=1)
    votes_h, fused_h = votes.cpu().numpy(), fused.cpu().numpy()
    print("end to end", ts, ": pixels in the band", int(in_band.sum()), "with a vote", int((ref["votes"] > 0).sum()), "of", votes_h.size)
    assert in_band.sum() <= pr.BAND_SHARE * in_band.size
    assert np.array_equal(votes_h[~in_band], ref["votes"][~in_band])
    keep = pr.valid(fused_h) & (votes_h >= 1) & seen
    assert not (keep & ~(pr.valid(depth) & seen)).any()           # a subset of the valid pixels
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                       # nothing is read on the host (the first call above warmed up)
    try:
        cloud = pc.reconstruct(model, inp, ts, window=WINDOW)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            xyz, rgb = cloud.points(0)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert len([c for c in caught if "synchroniz" in str(c.message)]) == 1      # one read
    pts = pc.unproject(fused, views["poses"], Kq, 256, window=WINDOW).cpu().numpy()
    assert xyz.tobytes() == pts[:, 0][keep[:, 0]].tobytes() and len(xyz) == keep.sum()
    assert np.array_equal(rgb, pr.compact(keep.astype(np.uint8), pts, views["rgb"].cpu().numpy())[1][0])
    assert int(cloud.count[0]) == len(xyz) and cloud.xyz.shape == (1, len(ts) * WINDOW[2] * WINDOW[3], 3)
    assert cloud.rgb.dtype == torch.uint8
    return cloud, xyz, rgb, ref


def test_reconstruct_end_to_end(dev, scene, tmp_path):
    from coponerf_amd import point_cloud as pc
    model, inp, views = scene
    y0, x0, h, w = WINDOW
    Kq = inp["query"]["intrinsics"]
    depth = views["depth"].cpu().numpy()
    seen = views["valid"].cpu().numpy() != 0

    # every valid pixel, unfused: cpn_depth_points' rows in (view, row, column) order
    cloud = pc.reconstruct(model, inp, TS, min_votes=0, fuse=False, window=WINDOW)
    xyz, rgb = cloud.points(0)
    raw = pc.unproject(views["depth"], views["poses"], Kq, 256, window=WINDOW).cpu().numpy()
    keep_all = pr.valid(depth) & seen
    assert xyz.tobytes() == raw[:, 0][keep_all[:, 0]].tobytes() and len(xyz) == keep_all.sum() > 0.05 * keep_all.size
    assert np.array_equal(rgb, pr.compact(keep_all.astype(np.uint8), raw, views["rgb"].cpu().numpy())[1][0])

    # the defaults on the two photos' own cameras.  The synthetic weights carry no geometry, so few pixels, or none, agree
    # across the two views; the same camera twice is the case in which they must: a pixel's point falls on the pixel itself
    # (to a rounding), and it gets its vote when the bilinear cell around it is in the window and valid
    _defaults_against_float64(model, inp, TS, dev)
    cloud, xyz, rgb, ref = _defaults_against_float64(model, inp, (0.0, 0.0), dev)
    inner = np.zeros((h, w), dtype=bool)
    inner[1:-1, 1:-1] = True                                      # its cell lies in the window whichever way the projection rounds
    ok = pr.valid(depth[0, 0]).reshape(h, w)
    if ok.all():
        assert (ref["votes"][0, 0].reshape(h, w)[inner] == 1).all()
    assert (ref["votes"] > 0).sum() > 0.05 * ref["votes"].size and len(xyz) > 0.05 * 2 * h * w

    path = tmp_path / "cloud.ply"
    cloud.save(path, 0)
    back_xyz, back_rgb = _parse_ply(path.read_bytes())
    assert back_xyz.tobytes() == xyz.tobytes() and np.array_equal(back_rgb, rgb)
