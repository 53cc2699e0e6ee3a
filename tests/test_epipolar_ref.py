"""The yardsticks of tests/epipolar_ref.py: the restated two_view_geometry against the reference's own output
(tests/golden/epipolar_F.npz), the integer coverage rules against brute force, the contour rule against scipy's erosion, the
margins and caps the GPU tests (tests/test_gpu_epipolar.py) rely on, and the wrappers' argument checks.  No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from coponerf_amd import summaries as sm
from tests import epipolar_ref as er

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "epipolar_F.npz")
SHAPES = ((1, 32), (3, 32), (1, 48), (3, 48), (2, 36))     # (B, S) of the GPU tests
FRINGE_CAP = 16                                            # pixels per line the steep case may leave undecided


def test_restated_geometry_reproduces_the_reference():
    gold = dict(np.load(GOLDEN))
    K, rel, gt = er.golden_inputs()
    assert np.array_equal(gold["intrinsics"], K.numpy()) and np.array_equal(gold["rel_pose"], rel.numpy())
    assert np.array_equal(gold["gt_rel_pose"], gt.numpy())
    E, F = er.two_view_geometry(K, rel, gt)
    for name, got in (("E", E[0]), ("F", F[0]), ("E_gt", E[1]), ("F_gt", F[1])):
        want = gold[name]
        assert want.dtype == np.float64 and want.shape == (4, 3, 3)
        worst = float(np.abs(got - want).max() / np.abs(want).max())
        print(name, "largest difference relative to the largest entry", worst)
        assert worst <= 1e-12, name
    assert er.inverse_margin(K) > 0                         # what tests/test_gpu_epipolar.py needs to compare F with the fixture
    assert not np.allclose(F[0], F[1], rtol=1e-3)           # the two kinds differ: the estimate is off the truth
    swapped = er.two_view_geometry(K.flip(1), rel, gt)[1]
    assert not np.allclose(F[0], swapped[0], rtol=1e-3)     # and so do the two orders of the views' intrinsics


def test_the_maker_reproduces_the_fixture(tmp_path):
    """Re-runs tests/golden/make_golden_epipolar.py where the reference it imports is present (a process of its own: the
    maker's stand-ins patch torch)."""
    from tests.golden import ref_shim
    if not os.path.isdir(ref_shim.REF):
        pytest.skip("the upstream reference is not on this machine")
    out = str(tmp_path / "again.npz")
    subprocess.run([sys.executable, os.path.join(HERE, "golden", "make_golden_epipolar.py"), out], check=True, capture_output=True)
    gold, again = dict(np.load(GOLDEN)), dict(np.load(out))
    assert sorted(gold) == sorted(again)
    for k in gold:
        if k in ("intrinsics", "rel_pose", "gt_rel_pose"):
            assert np.array_equal(gold[k], again[k]), k
        else:                                               # another CPU's LAPACK may round an inverse differently
            assert np.abs(gold[k] - again[k]).max() <= 1e-12 * np.abs(gold[k]).max(), k


def test_disc_half_widths():
    assert er.disc_half_widths(5) == [5, 4, 4, 4, 3, 0]
    assert er.disc_half_widths(2) == [2, 1, 0]
    assert er.disc_half_widths(0) == [0]


def test_integer_capsule_is_the_distance_test_outside_the_fringe():
    """200 seeded segments at S = 32, end points up to three image sides away, thickness 1 .. 12: the integer rule equals
    distance <= T / 2 on every pixel whose distance is further than 1e-9 from T / 2."""
    S, rng = 32, np.random.default_rng(2024)
    undecided = 0
    for i in range(200):
        p0, p1 = rng.integers(-3 * S, 4 * S, size=2), rng.integers(-3 * S, 4 * S, size=2)
        if i % 10 == 0:
            p1 = p0.copy()                                  # a segment of length 0: a disc of diameter T
        if i % 10 == 1:
            p0, p1 = rng.integers(0, S, size=2), rng.integers(0, S, size=2)        # both ends inside: the caps are visible
        T = int(rng.integers(1, 13))
        got = er.on_line(S, p0, p1, T)
        dist = er.brute_force_distance(S, p0, p1)
        clear = np.abs(dist - T / 2) > 1e-9
        undecided += int((~clear).sum())
        assert np.array_equal(got[clear], (dist <= T / 2)[clear]), (i, p0, p1, T)
        assert not (er.fringe(S, p0, p1, T) & clear & (np.abs(dist - T / 2) > 1e-6)).any()
    print("pixels at distance T / 2 to 1e-9:", undecided)


def test_contour_rule_is_the_region_minus_its_erosion():
    from scipy import ndimage
    cross = ndimage.generate_binary_structure(2, 1)
    for S in (8, 40):
        for name, mask in er.masks(S).items():
            region = mask == 0
            want = region & ~ndimage.binary_erosion(region, structure=cross, border_value=0)
            assert np.array_equal(er.contour_rule(mask), want), (S, name)
            drawn = er.draw_contour(np.full((S, S, 3), 7, np.uint8), mask)
            assert np.array_equal((drawn == er.CONTOUR_COLOR).all(-1), want) and bool((drawn[~want] == 7).all())
    assert not er.contour_rule(er.masks(8)["empty"]).any()
    full = er.contour_rule(er.masks(8)["full"])
    assert full.sum() == 28 and not full[1:-1, 1:-1].any()   # the image's own border
    assert er.contour_rule(er.masks(8)["pixel"]).sum() == 1
    assert er.contour_rule(er.masks(40)["diagonal"]).sum() == 16            # two 3 x 3 squares: all but their centres


@pytest.mark.parametrize("B,S", SHAPES)
def test_cases_decide_every_end_point(B, S):
    """What the GPU tests rely on: every case's end points lie further from an integer than both sides' roundings can move
    them, the lines do what the case is there for, and the steep case's fringe holds at most FRINGE_CAP pixels per line."""
    for name in er.CASES:
        ref = er.case_lines(name, B, S)
        valid, ends, margin = ref["valid"], ref["ends"], ref["margin"]
        rgb, K, _, _, points = er.case(name, B, S)
        P = len(points)
        assert er.inverse_margin(K) > 0, name               # both sides multiply the same fp32 inverses
        if name == "vertical":
            assert not valid.any() and bool((ref["lines"][..., 1] == 0).all())
            continue
        if name == "nan":
            bad = min(1, B - 1)
            assert not valid[0, bad].any() and not np.isfinite(ref["F"][0, bad]).all()
            keep = np.ones_like(valid)
            keep[0, bad] = False
            assert valid[keep].all() and float(margin[keep].min()) > 0
            continue
        assert valid.all(), name
        print(name, "smallest margin", float(margin.min()), "largest |y|", int(np.abs(ends[..., (1, 3)]).max()))
        assert float(margin.min()) > 0, name
        cover = np.stack([[[er.on_line(S, e[:2], e[2:], 10) for e in ends[k, b]] for b in range(B)] for k in range(2)])
        if name == "miss":
            assert not cover.any() and int(np.abs(ends).max()) <= 2 ** 15
        elif name == "steep":
            y = np.abs(ends[..., (1, 3)])
            assert int(y.min()) > 2 ** 16 and int(y.max()) < 2 ** 20
            assert cover.reshape(2, B, P, -1).any(-1).all()              # every line crosses the image
            for T in (3, 10):
                worst = max(int(er.fringe(S, e[:2], e[2:], T).sum()) for e in ends.reshape(-1, 4))
                print("steep: largest fringe of a line at thickness", T, "=", worst)
                assert worst <= FRINGE_CAP
        else:
            assert int(np.abs(ends).max()) <= 2 ** 15 and cover.reshape(2, B, P, -1).any(-1).all(), name
        if name == "shared":
            assert np.array_equal(ends[:, :, 0], ends[:, :, 2]) and not np.array_equal(ends[:, :, 0], ends[:, :, 1])
        if name == "same":
            assert np.array_equal(ends[0], ends[1])


def test_panels_reference_blends_and_orders():
    """The reference form on a hand case: the later point wins, the left half is unblended, the right half is
    0.4 colour + 0.6 image, untouched pixels keep their bits."""
    S = 16
    rgb = torch.zeros(1, 2, S, S, 3)
    rgb[:, 0] = 0.5
    points = [(4, 4), (5, 4)]
    colors = np.array([[10, 20, 30], [200, 100, 0]], dtype=np.float32)
    ends = np.array([[[[0, 8, S, 8], [0, 8, S, 8]]]] * 2)
    valid = np.ones((2, 1, 2), dtype=bool)
    valid[1, 0, 1] = False
    out, hit, delicate = er.panels(rgb, points, colors, ends, valid, 1, 2)
    assert hit[0, 0, 4, 4] == 1 and hit[0, 0, 4, 3] == 0 and hit[0, 0, 4, 6] == 1 and hit[0, 0, 0, 0] == -1
    assert out[0, 0, 4, 4].tolist() == [200, 100, 0] and out[0, 0, 0, 0].tolist() == [127.5] * 3
    assert sorted(set(np.nonzero(hit[0, 0, :, S:] >= 0)[0].tolist())) == [7, 8, 9]          # |dy| <= 1 = T / 2, no cap in sight
    assert np.array_equal(out[0, 0, 8, S + 3], np.float32(0.4) * colors[1] + np.float32(0.6) * np.float32(191.25))
    assert np.array_equal(out[1, 0, 8, S + 3], np.float32(0.4) * colors[0] + np.float32(0.6) * np.float32(191.25))
    assert delicate[0, 0, 7, S:].all() and not delicate[0, 0, 6, S:].any()                  # distance exactly T / 2
    assert np.array_equal(er.covered(out, rgb), hit >= 0)


def test_wrappers_refuse_host_tensors_and_bad_shapes():
    K, rel, gt = er.golden_inputs()
    pts = torch.tensor(sm.default_points(64), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="HIP device only"):
        sm.epipolar_lines(K, rel, gt, pts, 64)
    with pytest.raises(RuntimeError, match="HIP device only"):
        sm.epipolar_panels(torch.zeros(4, 2, 64, 64, 3), K, rel, gt)
    with pytest.raises(RuntimeError, match="HIP device only"):
        sm.mask_contour(torch.zeros(2, 8, 8, 3, dtype=torch.uint8), torch.zeros(2, 8, 8, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="HIP device only"):
        sm.flow_panels(torch.rand(1, 2, 8, 8, 3), (torch.rand(1, 2, 4, 4), torch.rand(1, 2, 4, 4)), contour=True)
    with pytest.raises(TypeError):
        sm.mask_contour([[0]], [[1]])
    with pytest.raises(TypeError):
        sm.epipolar_lines(K.numpy(), rel, gt, pts, 64)
    assert sm.EPIPOLAR_TAGS == ("epipolar_GT", "epipolar_pred") and not set(sm.EPIPOLAR_TAGS) & set(sm.IMAGE_TAGS)
    assert sm.default_points(256) == ((64, 64), (64, 128), (64, 192), (128, 64), (128, 128), (128, 192), (192, 64), (192, 128),
                                      (192, 192))
    assert len(sm.EPIPOLAR_COLORS) == 9 and sm.EPIPOLAR_COLORS[0] == (63, 228, 92) and sm.EPIPOLAR_COLORS[8] == (23, 240, 252)


def test_entry_points_check_arguments_before_any_launch():
    from coponerf_amd import _hip
    lib = _hip.lib()
    assert lib.cpn_epipolar_lines(None, None, None, None, 1, 9, 32, None, None, None, None, None) == -1
    assert b"null" in lib.cpn_last_error()
    assert lib.cpn_epipolar_lines(16, 16, 16, 16, 0, 9, 32, 16, 16, 16, 16, None) == -2
    assert lib.cpn_epipolar_lines(16, 16, 16, 16, 1, 0, 32, 16, 16, 16, 16, None) == -2
    assert lib.cpn_epipolar_lines(16, 16, 16, 16, 1, 9, 0, 16, 16, 16, 16, None) == -2
    assert lib.cpn_epipolar_panels(None, None, None, None, None, 1, 32, 9, 5, 10, None, None) == -1
    assert lib.cpn_epipolar_panels(16, 16, 16, 16, 16, 1, 0, 9, 5, 10, 16, None) == -2
    assert lib.cpn_epipolar_panels(16, 16, 16, 16, 16, 40000, 32, 9, 5, 10, 16, None) == -2
    assert lib.cpn_epipolar_panels(16, 16, 16, 16, 16, 1, 32, 9, 5, 0, 16, None) == -1 and b"thickness" in lib.cpn_last_error()
    assert lib.cpn_epipolar_panels(16, 16, 16, 16, 16, 1, 32, 9, 256, 10, 16, None) == -1
    assert lib.cpn_mask_contour(None, None, 1, 8, None, None) == -1
    assert lib.cpn_mask_contour(16, 16, 0, 8, 32, None) == -2 and lib.cpn_mask_contour(16, 16, 1, 0, 32, None) == -2
    assert lib.cpn_mask_contour(16, 16, 1, 8, 16, None) == -1 and b"must not be the overlay" in lib.cpn_last_error()
