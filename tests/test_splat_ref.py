"""tests/splat_ref.py pinned on the CPU: the restatements of csrc/splat.hip against a painter's implementation, the cases'
promises, the score against a direct float64 computation, orbit_poses, and the corner values of coverage and PSNR.  The GPU
tests (tests/test_gpu_splat.py) compare the kernels with these restatements exactly.
"""
import math

import numpy as np
import pytest
import torch

from coponerf_amd import _hip, splat
from tests import splat_ref as sr


# ---------------------------------------------------------------------------------------------------------------- painter
def _paint(case, radius):
    """The painter's algorithm, point by point in Python floats: the points that count, sorted by (z32, index) DESCENDING, each
    painting its whole footprint; the last write - the nearest point, the lower index among equal depths - wins.
    -> (index (K, B, H, W) int64, depth bits (K, B, H, W) uint32)."""
    H, W, K, B, cap = (case[k] for k in ("H", "W", "K", "B", "cap"))
    index = np.full((K, B, H, W), -1, dtype=np.int64)
    bits = np.full((K, B, H, W), 0x7FC00000, dtype=np.uint32)
    for k in range(K):
        for b in range(B):
            P = [[float(x) for x in row] for row in case["poses"][k, b]]
            Km = case["intrinsics"][b]
            fx, fy, cx, cy = float(Km[0, 0]), float(Km[1, 1]), float(Km[0, 2]), float(Km[1, 2])
            todo = []
            for i in range(min(max(int(case["count"][b]), 0), cap)):
                X = [float(x) for x in case["xyz"][b, i]]
                if not all(math.isfinite(x) for x in X):
                    continue
                d = [X[a] - P[a][3] for a in range(3)]
                Y = [(P[0][j] * d[0] + P[1][j] * d[1]) + P[2][j] * d[2] for j in range(3)]
                if not Y[2] >= sr.NEAR:
                    continue
                u, v = (fx * Y[0]) / Y[2] + cx, (fy * Y[1]) / Y[2] + cy
                z32 = np.float32(Y[2])
                if not (abs(u) < sr.LIM and abs(v) < sr.LIM and np.isfinite(z32)):
                    continue
                todo.append((float(z32), i, math.floor(u + 0.5), math.floor(v + 0.5), z32))
            for _, i, c, r, z32 in sorted(todo, key=lambda p: (p[0], p[1]), reverse=True):
                r0, r1, c0, c1 = max(r - radius, 0), min(r + radius, H - 1), max(c - radius, 0), min(c + radius, W - 1)
                if r0 <= r1 and c0 <= c1:
                    index[k, b, r0:r1 + 1, c0:c1 + 1] = i
                    bits[k, b, r0:r1 + 1, c0:c1 + 1] = z32.view(np.uint32)
    return index, bits


@pytest.mark.parametrize("name,radius", [("main", 0), ("main", 1), ("main", 2), ("pile", 0)])
def test_restatement_against_the_painter(name, radius):
    case = sr.all_cases()[name]
    got = sr.draw(case, radius, 0)
    index, bits = _paint(case, radius)
    assert np.array_equal(got["index"], index) and np.array_equal(got["bits"], bits)
    hit = index >= 0
    assert np.array_equal(got["zbuf"] == sr.EMPTY, ~hit)
    assert np.array_equal(got["zbuf"][hit], (bits[hit].astype(np.uint64) << np.uint64(32)) | index[hit].astype(np.uint64))
    for b in range(case["B"]):
        assert np.array_equal(got["frames"][:, b][hit[:, b]], case["rgb"][b][index[:, b][hit[:, b]]])
    assert (got["frames"][~hit] == 0).all()


def test_fill_takes_the_nearest_splatted_neighbour_once():
    case = sr.main_case()
    plain, filled = sr.draw(case, 0, 0), sr.draw(case, 0, 1, background=(9, 8, 7))
    H, W = case["H"], case["W"]
    changed = 0
    for k in range(case["K"]):
        for r in range(H):
            for c in range(W):
                own = plain["zbuf"][k, 0, r, c]
                want = own if own != sr.EMPTY else plain["zbuf"][k, 0, max(r - 1, 0):r + 2, max(c - 1, 0):c + 2].min()
                got = filled["index"][k, 0, r, c]
                assert got == (-1 if want == sr.EMPTY else int(want & np.uint64(0xFFFFFFFF)))
                changed += int(own == sr.EMPTY and want != sr.EMPTY)
    assert changed > 100                                                 # radius 0 leaves holes for the fill to close
    still = filled["index"][:, 0] < 0
    assert still.any() and (filled["frames"][:, 0][still] == (9, 8, 7)).all()      # and some it does not reach: no cascading


def test_cases_keep_their_promises():
    main = sr.main_case()
    assert (main["H"], main["W"], main["K"], main["B"], main["cap"]) == (24, 40, 3, 2, 600) and list(main["count"]) == [517, 0]
    for name, case in sr.all_cases().items():
        for radius in ((0, 1, 2) if name == "main" else (0,) if name == "pile" else (2,)):
            assert not sr.draw(case, radius, 0)["band"].any(), (name, radius)          # nothing near a threshold: nothing left out
    counts, c, r, z32, _ = sr.project(main["xyz"][0, :517], main["poses"][0, 0], main["intrinsics"][0], sr.NEAR)
    H, W = main["H"], main["W"]
    assert not counts[420:462].any()                                     # behind, nearer than near, not finite
    assert counts[:420].all() and counts[462:].all()
    outside = (c < 0) | (c >= W) | (r < 0) | (r >= H)
    assert outside[:406].sum() > 20 and outside[414:420].all()
    assert sorted(zip(c[406:414], r[406:414])) == sorted([(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, 0),
                                                          (W // 2, H - 1), (0, H // 2), (W - 1, H // 2)])
    for radius in (0, 1, 2):
        got = sr.draw(main, radius, 0)
        assert (got["index"][:, 1] == -1).all() and (got["index"] < 517).all()       # pair 1 empty; no row beyond the count
        for j in range(20):                                              # the pairs of equal depth: the first wins its pixel
            assert z32[462 + j].tobytes() == z32[482 + j].tobytes() and (c[462 + j], r[462 + j]) == (c[482 + j], r[482 + j])
            assert got["index"][0, 0, r[462 + j], c[462 + j]] == 462 + j
        dup = np.arange(0, 300, 20)
        seen = np.isin(got["index"][:, 0], dup).sum()
        assert seen > 0 and not np.isin(got["index"], 502 + np.arange(15)).any()     # of exact duplicates the earlier shows
    # cameras 1 and 2 see behind-camera, near and outside points of their own
    for k in (1, 2):
        ck = sr.project(main["xyz"][0, :517], main["poses"][k, 0], main["intrinsics"][0], sr.NEAR)[0]
        assert 400 < ck.sum() < 517 - 12
    # clipped footprints: the points just outside reach in at radius 1 or 2 only
    assert not np.isin(sr.draw(main, 0, 0)["index"][0], np.arange(414, 420)).any()
    assert np.isin(sr.draw(main, 1, 0)["index"][0, 0], [414, 415]).any() and np.isin(sr.draw(main, 2, 0)["index"][0, 0], [416, 417, 418, 419]).any()

    pile = sr.pile_case()
    got = sr.draw(pile, 0, 0)["index"][0, 0]
    assert got[sr.PILE_A[1], sr.PILE_A[0]] == pile["nearest"] and got[sr.PILE_B[1], sr.PILE_B[0]] == sr.PILE_N
    assert (got >= 0).sum() == 2
    wide = sr.wide_case()
    got = sr.draw(wide, 2, 0)["index"]
    assert (got > 65535).sum() > 50 and wide["cap"] > 256 * 256           # several workgroups; high indices win pixels


def test_score_against_a_direct_computation():
    case = sr.main_case()
    got = sr.draw(case, 1, 0)
    rng = np.random.default_rng(3)
    target = rng.integers(0, 256, size=got["frames"].shape, dtype=np.uint8)
    stats = sr.score(got["frames"], got["index"], target)
    for k in range(case["K"]):
        for b in range(case["B"]):
            hit = got["index"][k, b] >= 0
            diff = got["frames"][k, b][hit].astype(np.float64) - target[k, b][hit].astype(np.float64)
            assert stats[k, b, 0] == hit.sum() and stats[k, b, 1] == (diff ** 2).sum()
            cov, psnr = sr.coverage_psnr(stats, case["H"], case["W"])
            assert cov[k, b] == hit.mean()
            if hit.any():
                assert abs(psnr[k, b] - 10.0 * np.log10(255.0 ** 2 / (diff ** 2).mean())) < 1e-12
            else:
                assert np.isnan(psnr[k, b])
    assert (sr.score(got["frames"], got["index"], got["frames"])[..., 1] == 0).all()


def test_coverage_and_psnr_corner_values():
    stats = torch.tensor([[0, 0], [5, 0], [6, 6 * 3 * 255 ** 2], [24, 3 * 24], [24, 0]], dtype=torch.int64)
    cov, psnr = splat.coverage_psnr(stats, 4, 6)
    assert cov.dtype == torch.float64 and psnr.dtype == torch.float64
    assert cov.tolist() == [0.0, 5 / 24, 0.25, 1.0, 1.0]
    assert math.isnan(psnr[0]) and psnr[1] == math.inf and psnr[4] == math.inf        # nothing covered; covered and equal
    assert psnr[2] == 0.0 and abs(float(psnr[3]) - 20.0 * math.log10(255.0)) < 1e-12     # every byte off by 255; by 1
    want = sr.coverage_psnr(stats.numpy(), 4, 6)
    assert np.array_equal(cov.numpy(), want[0]) and np.allclose(psnr.numpy(), want[1], rtol=1e-15, atol=0, equal_nan=True)


def test_orbit_matrices():
    M = splat.orbit_matrices(7, 2.5, 40.0, pitch_deg=-10.0)
    assert M.shape == (7, 4, 4) and M.dtype == np.float64
    pivot = np.array([0.0, 0.0, 2.5])
    yaws = []
    for P in M:
        R, t = P[:3, :3], P[:3, 3]
        assert np.allclose(R @ R.T, np.eye(3), atol=1e-15) and abs(np.linalg.det(R) - 1.0) < 1e-15        # rigid
        assert np.array_equal(P[3], [0.0, 0.0, 0.0, 1.0])
        assert np.allclose(R.T @ (pivot - t), pivot, atol=1e-15)         # the pivot on the optical axis, at its distance
        yaws.append(np.degrees(np.arctan2(R[0, 2], R[2, 2])))
    assert np.allclose(yaws, np.linspace(-40.0, 40.0, 7), atol=1e-12)    # evenly over [-yaw, +yaw]
    assert np.array_equal(splat.orbit_matrices(5, 3.0, 0.0), np.broadcast_to(np.eye(4), (5, 4, 4)))      # yaw 0: the identity
    assert np.array_equal(splat.orbit_matrices(1, 3.0, 30.0)[0], np.eye(4))                             # one camera: the middle
    assert np.array_equal(splat.orbit_matrices(3, 3.0, 30.0)[1], np.eye(4))
    with pytest.raises(ValueError):
        splat.orbit_matrices(0, 3.0, 30.0)


def test_symbols_are_declared_with_their_types():
    import ctypes
    P, I, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    pr = _hip.PROTOTYPES
    assert pr["cpn_splat_points"] == (I, [P] * 4 + [I] * 6 + [D, P, P])
    assert pr["cpn_splat_resolve"] == (I, [P, P] + [I] * 7 + [P] * 4)
    assert pr["cpn_splat_score_scratch"] == (I, [I] * 4)
    assert pr["cpn_splat_score"] == (I, [P] * 3 + [I] * 4 + [P] * 3)
    assert _hip.CONSTANTS["SPLAT_SCORE_TILE"] == 4096 and _hip.ABI_VERSION == 12


def test_entry_checks_refuse_host_tensors():
    """Tiny CPU tensors of otherwise valid shape: a 2-point cloud, one camera, H = W = 4.  No library load."""
    from coponerf_amd.point_cloud import PointCloud
    cloud = PointCloud(torch.zeros(1, 2, 3), torch.zeros(1, 2, 3, dtype=torch.uint8), torch.full((1,), 2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="HIP device only"):
        splat.splat_points(cloud, torch.eye(4).expand(1, 1, 4, 4).contiguous(), torch.eye(4).expand(1, 4, 4).contiguous(), 4, 4)
    with pytest.raises(RuntimeError, match="one HIP device"):
        splat.resolve(torch.full((1, 1, 4, 4), -1, dtype=torch.int64), cloud.rgb)
    frames = torch.zeros(1, 1, 4, 4, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="one HIP device"):
        splat.score_counts(frames, torch.zeros(1, 1, 4, 4, dtype=torch.int32), frames)
