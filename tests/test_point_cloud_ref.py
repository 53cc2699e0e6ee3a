"""The yardsticks of tests/point_cloud_ref.py held to independent forms, on the CPU, before anything is compared with them:
the points to a matrix inverse, the votes to the scene's own geometry (ray casting), the compaction to boolean indexing, the
PLY bytes to a parser written here - and two conditions on the cases, so that no GPU test passes on an empty set."""
import numpy as np
import pytest

from coponerf_amd import point_cloud as pc
from tests import point_cloud_ref as pr


def _hom(P, X):
    """inv(P) [X; 1] with numpy's general inverse - not the [R^T | -R^T t] of the yardstick."""
    Pi = np.linalg.inv(np.asarray(P, dtype=np.float64))
    return X @ Pi[:3, :3].T + Pi[:3, 3]


def _smooth(case, k, b):
    """(h, w) bool: the pixel and its 8 neighbours lie on one surface and differ by at most 0.05 in depth."""
    h, w = case["h"], case["w"]
    d, s = case["true"][k, b].reshape(h, w), case["surface"][k, b].reshape(h, w)
    ok = np.zeros((h, w), dtype=bool)
    ok[1:-1, 1:-1] = True
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            dn, sn = np.roll(d, (dy, dx), (0, 1)), np.roll(s, (dy, dx), (0, 1))
            ok &= (sn == s) & (np.abs(dn - d) <= 0.05)
    return ok


def _second_difference(case, k, b):
    """(h, w): |d_xx| + |d_yy| + |d_xy| of the true depth by central differences (0 on the border)."""
    h, w = case["h"], case["w"]
    d = case["true"][k, b].reshape(h, w)
    out = np.zeros((h, w))
    c = d[1:-1, 1:-1]
    out[1:-1, 1:-1] = np.abs(d[1:-1, 2:] - 2 * c + d[1:-1, :-2]) + np.abs(d[2:, 1:-1] - 2 * c + d[:-2, 1:-1]) + \
        np.abs(d[2:, 2:] - d[2:, :-2] - d[:-2, 2:] + d[:-2, :-2]) / 4.0
    return out


def _visible_decisions(case):
    """(a, kb, b) -> bool (h w): the pixel of view a is seen by view kb away from every silhouette - its true point projects
    between four taps of kb that are smooth and on the pixel's own surface, and kb's own ray through that projection hits
    the scene at that very point (nothing in front of it).  From the scene's geometry alone."""
    K, B = case["depth"].shape[:2]
    y0, x0, h, w = pr.window_of(case["S"], case["window"])
    u, v = pr.pixel_grid(case["S"], case["window"])
    out = {}
    for b in range(B):
        cam = pr.cam_of(case["intrinsics"][b])
        for a in range(K):
            d = case["true"][a, b]
            P = case["poses"][a, b].astype(np.float64)
            X = np.stack(pr.on_ray(cam, u, v, d), axis=-1) @ P[:3, :3].T + P[:3, 3]
            own = _smooth(case, a, b).reshape(-1)
            for kb in range(K):
                if kb == a:
                    continue
                Y = _hom(case["poses"][kb, b], X)
                qx, qy = cam[0] * Y[:, 0] / Y[:, 2] + cam[2], cam[1] * Y[:, 1] / Y[:, 2] + cam[3]
                ix, iy = np.floor(qx - x0).astype(int), np.floor(qy - y0).astype(int)
                inside = (ix >= 0) & (ix + 1 <= w - 1) & (iy >= 0) & (iy + 1 <= h - 1)
                ixc, iyc = np.clip(ix, 0, w - 2), np.clip(iy, 0, h - 2)
                sm, sf = _smooth(case, kb, b), case["surface"][kb, b].reshape(h, w)
                same = np.ones_like(inside)
                for dy in (0, 1):
                    for dx in (0, 1):
                        same &= sm[iyc + dy, ixc + dx] & (sf[iyc + dy, ixc + dx] == case["surface"][a, b])
                hit, _ = pr.cast(case["poses"][kb, b], cam, qx, qy)
                out[(a, kb, b)] = own & inside & same & (np.abs(hit - Y[:, 2]) <= 1e-9 * np.abs(hit))
    return out


def test_points_reproject_to_their_pixels():
    case = pr.clean_case()
    xyz, bound = pr.depth_points(case["depth"], case["poses"], case["intrinsics"], case["S"], case["window"])
    u, v = pr.pixel_grid(case["S"], case["window"])
    assert np.isfinite(xyz).all() and (bound > 0).all() and (bound < 1e-6).all()
    for k in range(3):
        for b in range(2):
            fx, fy, cx, cy = pr.cam_of(case["intrinsics"][b])
            Y = _hom(case["poses"][k, b], xyz[k, b])
            assert np.abs(fx * Y[:, 0] / Y[:, 2] + cx - u).max() <= 1e-12
            assert np.abs(fy * Y[:, 1] / Y[:, 2] + cy - v).max() <= 1e-12
            assert np.abs(Y[:, 2] - case["depth"][k, b].astype(np.float64)).max() <= 1e-12


def test_clean_scene_every_visible_pixel_gets_its_vote():
    case = pr.clean_case()
    res = pr.votes_of(case)
    seen = _visible_decisions(case)
    n_seen = 0
    for (a, kb, b), vis in seen.items():
        assert res["consistent"][a, kb, b][vis].all(), (a, kb, b)
        n_seen += int(vis.sum())
    assert n_seen >= 0.4 * res["decided"].sum()                  # the statement covers a large part of the scene, not a corner
    assert (res["votes"] == res["consistent"].sum(axis=1)).all() and res["votes"].max() == 2


def test_clean_scene_fused_depth_is_the_true_depth():
    """Where every other view sees the pixel, depth_fused is the true depth up to what the rule itself adds: the bilinear
    lookup of a depth map that is not bilinear (a plane's depth is a rational function of the pixel; the error of a bilinear
    interpolant is at most (|d_xx| + |d_yy|) / 8 + |d_xy| / 4 of the cell, taken here as half the largest second difference
    of the taps' view), and the fp32 rounding of the ray-cast depths, 4 U d with d < 10 for the two depths and two poses."""
    case = pr.clean_case()
    res = pr.votes_of(case)
    seen = _visible_decisions(case)
    checked = 0
    for b in range(2):
        for a in range(3):
            others = [kb for kb in range(3) if kb != a]
            vis = np.logical_and.reduce([seen[(a, kb, b)] for kb in others])
            curve = max(_second_difference(case, kb, b)[_smooth(case, kb, b)].max() for kb in others)
            err = np.abs(res["fused"][a, b] - case["true"][a, b])[vis]
            assert err.max() <= 0.5 * curve + 4 * pr.U * 10, (a, b, err.max(), curve)
            assert (res["votes"][a, b][vis] == 2).all()
            checked += int(vis.sum())
    assert checked > 2000


def test_main_case_planted_faults():
    case = pr.main_case()
    K, B, h, w = 3, 2, case["h"], case["w"]
    res = pr.votes_of(case)
    xyz, _ = pr.depth_points(case["depth"], case["poses"], case["intrinsics"], case["S"], case["window"])
    votes, fused = res["votes"].reshape(K, B, h, w), res["fused"].reshape(K, B, h, w)
    nan_pts = np.isnan(xyz).reshape(K, B, h, w, 3)
    assert (nan_pts.all(axis=-1) == nan_pts.any(axis=-1)).all()
    bad = ~pr.valid(case["depth"]).reshape(K, B, h, w)
    for view, rows, cols in ((0, 2, slice(None)), (1, 33, slice(None)), (2, 5, slice(None)), (2, 20, 40)):   # NaN, 0, 10, +inf
        assert bad[view, :, rows, cols].all()
    assert bad.sum() == B * (3 * w + 1)
    assert (nan_pts.all(axis=-1) == bad).all() and (votes[bad] == 0).all() and np.isnan(fused[bad]).all()
    assert np.isfinite(fused[~bad]).all()
    # the patch scaled by 1.2 loses every vote; around it the scene keeps them
    assert (votes[pr.PATCH[0], :, pr.PATCH[1], pr.PATCH[2]] == 0).all()
    clean = pr.votes_of(pr.clean_case())["votes"].reshape(K, B, h, w)
    assert (clean[pr.PATCH[0], :, pr.PATCH[1], pr.PATCH[2]] > 0).mean() > 0.8
    # the near depths of view 0 lie behind camera 2 and in front of camera 1
    view, row, cols = pr.NEAR_ROW
    behind = res["behind"].reshape(K, K, B, h, w)
    assert behind[view, 2, :, row, cols].all() and not behind[view, 1, :, row, cols].any()
    assert not pr.votes_of(pr.clean_case())["behind"].any()
    # the sphere's silhouette is in the window: a depth edge
    assert 0.02 < case["surface"].mean() < 0.5


def test_one_view_has_no_votes():
    case = pr.further_cases()["K1"]
    res = pr.votes_of(case)
    ok = pr.valid(case["depth"])
    assert not res["votes"].any() and not res["decided"].any()
    assert np.array_equal(res["fused"][ok], case["depth"][ok].astype(np.float64)) and np.isnan(res["fused"][~ok]).all()


@pytest.mark.parametrize("name", ["main", "K1", "K2", "whole"])
def test_cases_are_decided_away_from_the_thresholds(name):
    """At most BAND_SHARE of the (a, b, pixel) decisions lie within BAND of a threshold: a GPU test that leaves the band out
    still compares (nearly) everything."""
    res = pr.votes_of(pr.all_cases()[name])
    n = int(res["decided"].sum())
    assert int(res["near"].sum()) <= pr.BAND_SHARE * max(n, 1)
    assert (n == 0) == (name == "K1")


def test_main_case_decides_both_ways():
    res = pr.votes_of(pr.main_case())
    share = res["consistent"].sum() / res["decided"].sum()
    print("consistent share of the main case", share)
    assert 0.2 <= share <= 0.8
    for name in ("K2", "whole"):
        r = pr.votes_of(pr.further_cases()[name])
        assert 0 < r["consistent"].sum() < r["decided"].sum()


def test_compaction_is_boolean_indexing():
    rng = np.random.default_rng(3)
    K, B, R = 3, 2, 37 * 53
    xyz = rng.normal(size=(K, B, R, 3)).astype(np.float32)
    rgb = pr.colours((K, B, R, 3))
    for keep in (rng.integers(0, 2, size=(K, B, R)).astype(np.uint8) * 255, np.ones((K, B, R), np.uint8), np.zeros((K, B, R), np.uint8)):
        ox, oc, n = pr.compact(keep, xyz, rgb)
        for b in range(B):
            m = keep[:, b].astype(bool)
            assert n[b] == m.sum() and np.array_equal(ox[b], xyz[:, b][m])
            with np.errstate(invalid="ignore"):
                want = np.rint(np.clip((rgb[:, b][m].astype(np.float64) + 1) * 127.5, 0, 255))
            want = np.where(np.isnan(want), 0, want).astype(np.uint8)
            # the float64 form and the fp32 rule can only differ where (x + 1) * 127.5 rounds onto a tie in fp32
            assert (oc[b] != want).sum() <= 1e-3 * want.size and np.abs(oc[b].astype(int) - want).max(initial=0) <= 1
            assert (oc[b][np.isnan(rgb[:, b][m])] == 0).all()


def _parse_ply(data):
    """(xyz (n, 3) float32, rgb (n, 3) uint8) of a binary little-endian PLY of float x y z, uchar red green blue vertices."""
    head, _, body = data.partition(b"end_header\n")
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0" and lines[-1] == ""
    assert lines[2].startswith("element vertex ")
    n = int(lines[2].split()[2])
    props = [tuple(line.split()[1:]) for line in lines[3:-1]]
    assert props == [("float", "x"), ("float", "y"), ("float", "z"), ("uchar", "red"), ("uchar", "green"), ("uchar", "blue")]
    assert len(body) == 15 * n
    rows = np.frombuffer(body, dtype=np.uint8).reshape(n, 15)
    return rows[:, :12].copy().view("<f4").reshape(n, 3), rows[:, 12:].copy()


@pytest.mark.parametrize("n", [0, 1, 1000])
def test_ply_bytes_parse_back(n, tmp_path):
    rng = np.random.default_rng(n)
    xyz = rng.normal(size=(n, 3)).astype(np.float32)
    rgb = rng.integers(0, 256, size=(n, 3)).astype(np.uint8)
    got_xyz, got_rgb = _parse_ply(pc.ply_bytes(xyz, rgb))
    assert np.array_equal(got_xyz, xyz) and np.array_equal(got_rgb, rgb)
    with pytest.raises(ValueError):
        pc.ply_bytes(xyz.astype(np.float64), rgb)


def test_new_symbols_are_declared():
    from coponerf_amd import _hip
    for name in ("cpn_depth_points", "cpn_depth_votes", "cpn_compact_points", "cpn_compact_points_scratch"):
        assert name in _hip.PROTOTYPES
    assert _hip.ABI_VERSION == 12 and _hip.CONSTANTS["COMPACT_TILE"] % _hip.CONSTANTS["COMPACT_FINISH"] == 0


def test_entry_checks_refuse_host_tensors():
    """Tiny CPU tensors of otherwise valid shape: K = 2 views of a 4 x 4 grid.  No library load."""
    import torch
    depth, poses, intr = torch.ones(2, 1, 16), torch.eye(4).expand(2, 1, 4, 4).contiguous(), torch.eye(4).expand(1, 4, 4).contiguous()
    with pytest.raises(RuntimeError, match="HIP device only"):
        pc.unproject(depth, poses, intr, 4)
    with pytest.raises(RuntimeError, match="HIP device only"):
        pc.vote(depth, poses, intr, 4, 1.0, 0.01)
    with pytest.raises(RuntimeError, match="one HIP device"):
        pc.compact(torch.ones(2, 1, 16, dtype=torch.uint8), torch.zeros(2, 1, 16, 3), torch.zeros(2, 1, 16, 3), 4, 4)
