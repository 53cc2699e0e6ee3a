"""The yardsticks of tests/novel_views_ref.py held to independent ones, on the CPU: the resample rule to F.interpolate in
float64, the camera path to scipy's Slerp, the intrinsics to the loader's, and the host side of coponerf_amd/novel_views.py
(no device is touched)."""
import numpy as np
import pytest
import torch

from coponerf_amd import _hip, novel_views as nv
from coponerf_amd.shards import crop_window, sample_intrinsics
from tests import novel_views_ref as nr


# ----------------------------------------------------------------------------------------------------------- the resample
@pytest.mark.parametrize("shape,size", nr.FIT_CASES)
@pytest.mark.parametrize("antialias", (True, False))
def test_resample_rule_is_interpolate_in_float64(shape, size, antialias):
    noise, const, _ = nr.fit_case(*shape, size)
    for img in (noise[:1], const[:1]):
        got, want = nr.resample64(img, size, antialias), nr.interpolate64(img, size, antialias)
        err = float(np.abs(got - want).max())
        print(shape, size, antialias, err)
        assert err <= 1e-11


def test_resample_rule_at_the_sizes_of_the_issue():
    """36 -> 16, 8 -> 16, 360 -> 256 and 1000 -> 32 as one axis; the flag matters at 360 -> 256."""
    for n_in, n_out in ((36, 16), (8, 16), (360, 256), (1000, 32)):
        img = (nr.syn._bits(n_in * n_in * 3, 7, n_in) >> np.uint64(56)).astype(np.uint8).reshape(1, n_in, n_in, 3)
        for aa in (True, False):
            assert np.abs(nr.resample64(img, n_out, aa) - nr.interpolate64(img, n_out, aa)).max() <= 1e-11
        if n_in == 360:
            assert np.abs(nr.resample64(img, n_out, True) - nr.resample64(img, n_out, False)).max() > 50


def test_identity_weights_are_exactly_one():
    for aa in (True, False):
        W, T = nr.axis_weights(16, 16, aa)
        assert np.array_equal(W, np.eye(16)) and T == 2      # the second tap of a row has weight exactly 0
    _, T = nr.axis_weights(700, 32, True)
    assert T > 40
    assert nr.axis_weights(8192, 256, True)[1] > 60


def test_fit_bound_counts_taps():
    """To first order the bound is (8 T + 11) U: 2 gamma(4 T + 4) + 3 U, plus the float64 term."""
    for (Hi, Wi), size in nr.FIT_CASES:
        for aa in (True, False):
            side = crop_window(Hi, Wi)[2]
            T = nr.axis_weights(side, size, aa)[1]
            b = nr.fit_bound(Hi, Wi, size, aa)
            assert (8 * T + 11) * nr.U <= b <= (8 * T + 12) * nr.U * 1.001, (Hi, Wi, size, aa, T, b)
    assert nr.fit_bound(1000, 700, 32, True) < 3e-5          # 45 taps: still far below half a grey level (3.9e-3)


# --------------------------------------------------------------------------------------------------------------- the path
def test_path_is_slerp_and_linear_translation():
    from scipy.spatial.transform import Rotation, Slerp
    rng = np.random.default_rng(5)
    ts = np.array([0.0, 0.125, 0.5, 0.9, 1.0])
    for angle in (1e-9, 0.3, 1.2, 1.7, 2.5, 3.1):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        rot = Rotation.from_rotvec(axis * angle)
        rel = np.eye(4)
        rel[:3, :3], rel[:3, 3] = rot.as_matrix(), rng.normal(size=3)
        got = nr.path64(rel[None], ts)[:, 0]
        want = Slerp([0.0, 1.0], Rotation.concatenate([Rotation.identity(), rot]))(ts).as_matrix()
        assert np.abs(got[:, :3, :3] - want).max() <= 1e-12, angle
        assert np.abs(got[:, :3, 3] - ts[:, None] * rel[:3, 3]).max() <= 1e-12
        for t in (-0.25, 1.5):                               # Slerp does not extrapolate: the rotation vector does
            want = Rotation.from_rotvec(axis * angle * t).as_matrix()
            assert np.abs(nr.power_of_rotation(rel[:3, :3], t) - want).max() <= 1e-12, (angle, t)


def test_path_ends_and_small_angles():
    R = nr.rotation_about((0.3, -1.0, 0.2), 0.7)
    assert np.array_equal(nr.power_of_rotation(R, 0.0), np.eye(3))
    assert np.array_equal(nr.power_of_rotation(R, 1.0), R)
    assert np.array_equal(nr.power_of_rotation(np.eye(3), 0.4), np.eye(3))                 # angle 0
    assert np.array_equal(nr.power_of_rotation(nr.rotation_about((0, 0, 1), 1e-13), 0.4), np.eye(3))


def test_path_near_half_a_turn_is_finite_and_orthonormal():
    for axis in ((1.0, -0.4, 0.7), (0.0, 0.0, 1.0), (1e-3, 1.0, 1e-3)):
        R = nr.rotation_about(axis, np.pi - 1e-9)
        for t in (-0.25, 0.3, 0.5, 1.5):
            Q = nr.power_of_rotation(R, t)
            assert np.isfinite(Q).all()
            assert np.abs(Q @ Q.T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(Q) - 1.0) <= 1e-12
            want = nr.rotation_about(axis, (np.pi - 1e-9) * t)
            assert np.abs(Q - want).max() <= 1e-9            # the axis is well determined from the symmetric part


def test_sway_is_a_circle_in_the_camera_frame():
    rel = np.eye(4)
    rel[:3, :3], rel[:3, 3] = nr.rotation_about((0, 1, 0), 0.4), (0.5, 0.0, 0.1)
    ts = np.linspace(0, 1, 9)
    plain, swayed = nr.path64(rel[None], ts)[:, 0], nr.path64(rel[None], ts, sway=0.05, turns=2.0)[:, 0]
    assert np.array_equal(plain[:, :3, :3], swayed[:, :3, :3])
    local = np.einsum("kji,kj->ki", plain[:, :3, :3], swayed[:, :3, 3] - plain[:, :3, 3])   # R^T (offset)
    assert np.abs(local[:, 2]).max() <= 1e-15 and np.abs(np.hypot(local[:, 0], local[:, 1]) - 0.05).max() <= 1e-15
    assert np.allclose(local[4, :2], (0.05, 0.0), atol=1e-15)                               # t = 0.5, two turns: a full circle


# --------------------------------------------------------------------------------------------------------- the intrinsics
def test_intrinsics_equal_the_loaders_at_256_by_455():
    for fx, fy in ((0.5, 0.89), (0.4871, 0.8659), (1.0 / 3.0, 0.7)):
        K_px = np.array([[fx * 455, 0, 0.5 * 455], [0, fy * 256, 0.5 * 256], [0, 0, 1]])
        got = nv.fit_intrinsics(K_px, 256, 455, 256).astype(np.float32)
        assert np.array_equal(got, sample_intrinsics(np.array([fx, fy, 0.5, 0.5]), 256, 455))


def test_intrinsics_follow_the_crop_and_the_scale():
    K = nv.fit_intrinsics(nv.hfov_intrinsics(90.0, 1000, 700), 1000, 700, 256)
    s = 256 / 700
    assert np.allclose(K[:3, :3], [[350 * s, 0, 128], [0, 350 * s, 128], [0, 0, 1]], rtol=1e-15)
    K = nv.fit_intrinsics([[500.0, 0, 30.0], [0, 510.0, 20.0], [0, 0, 1]], 37, 53, 18)       # crop side 36, offset (0.5, 8.5)
    assert np.allclose(K[:3, :3], [[250.0, 0, (30 - 8.5) / 2], [0, 255.0, (20 - 0.5) / 2], [0, 0, 1]], rtol=1e-15)
    assert np.array_equal(K[3], (0, 0, 0, 1)) and np.array_equal(K[:3, 3], (0, 0, 0))


# --------------------------------------------------------------------------------------------------------------- the pack
def test_pack_rule_on_its_corner_values():
    special, ties = nr.pack_values()
    assert len(ties) >= 3 and np.float32(0.0) in ties
    got = nr.pack_rule(special.reshape(1, -1, 1).repeat(3, axis=2), 1, len(special))[0, 0, :, 0]
    assert got.tolist() == [0, 255, 0, 128, 128, 255, 0, 0, 255, 1]
    g = (ties + np.float32(1)) * np.float32(127.5)
    assert np.array_equal(nr.to_byte(g), (2 * np.round(g.astype(np.float64) / 2)).astype(np.uint8))   # ties go to the even byte
    d = np.array([[np.nan, -1.0, 0.0, 5.0, 10.0, 12.0]], dtype=np.float32)
    panel = nr.pack_rule(np.zeros((1, 6, 3), np.float32), 1, 6, depth=d)
    table = np.rint(nr.jet_table().astype(np.float32) * np.float32(255)).astype(np.uint8)
    assert panel.shape == (1, 1, 12, 3) and np.array_equal(panel[0, 0, :6], np.full((6, 3), 128, np.uint8))
    assert np.array_equal(panel[0, 0, 6:], np.stack([np.zeros(3, np.uint8), table[0], table[0], table[128], table[255], table[255]]))


# ------------------------------------------------------------------------------------------------------- the host interface
def test_entry_points_are_declared_and_the_version_stays():
    for name in ("cpn_fit_images_u8", "cpn_camera_path", "cpn_pack_frames"):
        assert name in _hip.SIGNATURES
    assert len(_hip.SIGNATURES["cpn_fit_images_u8"]) == 12 and len(_hip.SIGNATURES["cpn_camera_path"]) == 8
    assert len(_hip.SIGNATURES["cpn_pack_frames"]) == 8
    assert _hip.ABI_VERSION == 12


def test_argument_checks_need_no_device():
    img = np.zeros((8, 8, 3), np.uint8)
    with pytest.raises(ValueError, match="exactly one"):
        nv.prepare_pair(img, img)
    with pytest.raises(ValueError, match="exactly one"):
        nv.prepare_pair(img, img, intrinsics=np.eye(3), hfov_deg=60.0)
    with pytest.raises(ValueError, match="uint8"):
        nv.prepare_pair(img.astype(np.float32), img, hfov_deg=60.0)
    with pytest.raises(ValueError, match=r"\(Hi, Wi, 3\)"):
        nv.prepare_pair(np.zeros((8, 8), np.uint8), img, hfov_deg=60.0)
    with pytest.raises(RuntimeError, match="HIP device"):
        nv.camera_path(torch.eye(4)[None], [0.5])
