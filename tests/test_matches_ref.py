"""tests/matches_ref.py against independent forms, on the CPU: the numpy restatements the GPU tests of coponerf_amd.matches compare
the kernels with must themselves be right, their bounds must catch seeded defects, and the inputs must keep the share of
pixels near a threshold under the cap.  Also the host parts of coponerf_amd/matches.py: photo_coords and the packing of
Matches.numpy.
"""
import numpy as np
import pytest
import torch

from coponerf_amd import matches as mt
from coponerf_amd.aux_outputs import cycle_masks
from coponerf_amd.novel_views import fit_intrinsics
from tests import matches_ref as mr

SMALL = ((2, 32, 8), (2, 24, 8))                                 # (B, S, h): scale 4, and scale 3 (h / S is not an fp32 number)
LARGE = (2, 256, 64)


# ------------------------------------------------------------------------------------------------------------ match fields
@pytest.mark.parametrize("B,S,h", SMALL + (LARGE,))
def test_inputs_keep_the_band_small_and_the_mask_mixed(B, S, h):
    ref = mr.fields_ref(B, S, h)
    mask, far = mr.mask_of(ref)
    print(S, "mask", mask.mean(), "inside", ref["inside"].mean(), "band", 1 - far.mean())
    assert 0.20 <= mask.mean() <= 0.75
    assert 1.0 - far.mean() <= mr.BAND_SHARE
    assert (~ref["inside"]).mean() > 0.1                          # some matches leave the image
    assert np.isnan(ref["cycle"]).any() and np.isnan(ref["q"]).any()               # the NaN flow entry is seen
    assert not np.isnan(ref["q"][1]).any()                         # and stays in its own direction's matches
    # the fp32 sequence and the float64 values of the same rule agree within the bound derived for the kernel
    ok = ~np.isnan(ref["q"])
    assert (np.abs(ref["q32"].astype(np.float64) - ref["q"])[ok] <= ref["q_bound"][ok]).all()


def test_mask_equals_cycle_masks_on_cpu_tensors():
    """(cycle <= 10) & inside is aux_outputs.cycle_masks - the stock-op chain on CPU tensors - on every pixel whose decisions are
    at least 1e-3 px from their thresholds."""
    B, S, h = LARGE
    f0, f1, _, _ = mr.fields_case(B, S, h)
    ref = mr.fields_ref(B, S, h)
    mask, far = mr.mask_of(ref)
    m1, m2 = cycle_masks((torch.from_numpy(f0.copy()), torch.from_numpy(f1.copy())), h)
    stock = np.stack((m1.numpy().astype(bool), m2.numpy().astype(bool)))
    assert stock.shape == mask.shape
    print("mask pixels", int(mask.sum()), "differing inside the band", int((stock != mask)[~far].sum()))
    assert np.array_equal(stock[far], mask[far])


@pytest.mark.parametrize("B,S,h", SMALL)
def test_epi_against_the_textbook_sampson_distance(B, S, h):
    """F = inv(K0)^T [t]x R inv(K1) with numpy.linalg.inv of the 3 x 3 intrinsics, and
    x0^T F x1 / sqrt((F x1)_0^2 + (F x1)_1^2 + (F^T x0)_0^2 + (F^T x0)_1^2) on homogeneous pixels."""
    _, _, K, P = mr.fields_case(B, S, h)
    ref = mr.fields_ref(B, S, h)
    q = ref["q32"].astype(np.float64)
    py, px = np.mgrid[0:S, 0:S].astype(np.float64)
    worst = 0.0
    for b in range(B):
        R, t = P[b, :3, :3].astype(np.float64), P[b, :3, 3].astype(np.float64)
        tx = np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])
        Fm = np.linalg.inv(K[b, 0, :3, :3].astype(np.float64)).T @ tx @ R @ np.linalg.inv(K[b, 1, :3, :3].astype(np.float64))
        for d in range(2):
            p = np.stack((px, py, np.ones_like(px)), -1)
            m = np.concatenate((q[d, b], np.ones((S, S, 1))), -1)
            x0, x1 = (p, m) if d == 0 else (m, p)
            Fx1, Ftx0 = x1 @ Fm.T, x0 @ Fm
            want = (x0 * Fx1).sum(-1) / np.sqrt(Fx1[..., 0] ** 2 + Fx1[..., 1] ** 2 + Ftx0[..., 0] ** 2 + Ftx0[..., 1] ** 2)
            ok = ~np.isnan(want)
            assert np.array_equal(np.isnan(ref["epi"][d, b]), ~ok)
            worst = max(worst, float(np.abs(want - ref["epi"][d, b])[ok].max()))
    print("epi against the textbook form: largest difference", worst, "px")
    assert worst <= 1e-10                                         # two float64 forms of a value of a few pixels


def test_epi_vanishes_on_true_correspondences_with_the_sign_convention():
    sc = mr.refine_scene()
    P = np.eye(4)
    P[:3, :3], P[:3, 3] = sc["R_true"], sc["t_true"]
    k0, k1 = mr.cam_of(sc["intrinsics"][0]), mr.cam_of(sc["intrinsics"][1])
    xy = sc["xy"].astype(np.float64)
    r, ok = mr.residual(mr.sampson(mr.essential(P[:3, :3], P[:3, 3]), k0, k1, *(xy[:, i] for i in range(4))))
    assert ok.all() and np.abs(r).max() < 1e-4                    # fp32 coordinates: 1.5e-5 px each
    r_t, _ = mr.residual(mr.sampson(mr.essential(P[:3, :3].T, -P[:3, :3].T @ P[:3, 3]), k0, k1, *(xy[:, i] for i in range(4))))
    assert np.abs(r_t).max() > 1.0                                # the inverse pose is not the convention


def test_defects_in_the_fields_are_caught_by_their_bounds():
    B, S, h = SMALL[0]
    f0, f1, K, P = mr.fields_case(B, S, h)
    ref = mr.fields_ref(B, S, h)
    swapped, _ = mr.epi_field(ref["q32"], K, P, defect="swapped direction")
    ok = ~np.isnan(ref["epi"][1])
    assert (np.abs(swapped - ref["epi"])[1][ok] > ref["epi_bound"][1][ok]).mean() > 0.99
    assert np.array_equal(swapped[0], ref["epi"][0], equal_nan=True)
    clamped = mr.match_fields(f0, f1, K, P, S, defect="tap outside")
    both = np.isfinite(clamped["cycle"]) & np.isfinite(ref["cycle"])
    caught = np.abs(clamped["cycle"] - ref["cycle"])[both] > ref["cycle_bound"][both]
    print("a tap read outside: pixels beyond the bound", int(caught.sum()), "of", int(both.sum()))
    assert caught.sum() > 0.1 * both.sum()


# -------------------------------------------------------------------------------------------------------------- compaction
def test_compact_is_boolean_indexing_and_an_off_by_one_shows():
    B, S, h = SMALL[0]
    ref = mr.fields_ref(B, S, h)
    mask, _ = mr.mask_of(ref)
    keep = mr.stride_keep(mask, 2).astype(np.uint8)
    q32, cyc, epi = ref["q32"], ref["cycle"].astype(np.float32), ref["epi"].astype(np.float32)
    xy, err, n = mr.compact(keep, q32, cyc, epi)
    py, px = np.mgrid[0:S, 0:S]
    for b in range(B):
        k0, k1 = keep[0, b] != 0, keep[1, b] != 0
        assert n[b] == k0.sum() + k1.sum() > 0
        assert np.array_equal(xy[b][:k0.sum(), 0], px[k0]) and np.array_equal(xy[b][:k0.sum(), 1], py[k0])       # view 0's own pixels
        assert np.array_equal(xy[b][:k0.sum(), 2:], q32[0, b][k0])
        assert np.array_equal(xy[b][k0.sum():, 2], px[k1]) and np.array_equal(xy[b][k0.sum():, :2], q32[1, b][k1])
        assert np.array_equal(err[b][:, 0], np.concatenate((cyc[0, b][k0], cyc[1, b][k1])))
        assert np.array_equal(err[b][:, 1], np.concatenate((epi[0, b][k0], epi[1, b][k1])), equal_nan=True)
    bad = mr.compact(keep, q32, cyc, epi, defect="order")
    assert all(a.tobytes() != b.tobytes() for a, b in zip(xy, bad[0])) and np.array_equal(n, bad[2])


def test_pack_and_unpack_of_one_pair():
    rng = np.random.default_rng(3)
    cap = 37
    xy, err = rng.normal(size=(cap, 4)).astype(np.float32), rng.normal(size=(cap, 2)).astype(np.float32)
    for n in (0, 1, 20, cap):
        packed = mt.pack_matches(torch.tensor([n], dtype=torch.int32), torch.from_numpy(xy), torch.from_numpy(err))
        assert packed.dtype == torch.uint8 and packed.numel() == 4 + 24 * cap
        a, b = mt.unpack_matches(packed.numpy(), cap)
        assert a.shape == (n, 4) and b.shape == (n, 2) and a.dtype == b.dtype == np.float32
        assert a.tobytes() == xy[:n].tobytes() and b.tobytes() == err[:n].tobytes()


# -------------------------------------------------------------------------------------------------------------- refinement
def test_block_sum_and_the_solve_are_what_they_say():
    rng = np.random.default_rng(5)
    for n in (1, 7, 256, 1000):
        terms = rng.normal(size=(n, 30))
        got = mr.block_sum(terms)
        assert np.abs(got - terms.sum(0)).max() <= 64 * mr.E * np.abs(terms).sum(0).max()
    M = rng.normal(size=(6, 6))
    A, g = M @ M.T + 0.1 * np.eye(6), rng.normal(size=6)
    assert np.abs(mr.solve6(A, g) - np.linalg.solve(A, -g)).max() <= 1e-12 * np.linalg.cond(A)
    assert mr.solve6(A - 10 * np.eye(6), g) is None               # not positive definite
    A[2, 2] = np.nan
    assert mr.solve6(A, g) is None


def test_jacobian_against_finite_differences():
    """g = sum w J r of a pass is the gradient of the cost's Gauss-Newton model; the rows J themselves are checked here against
    central differences of the residual under R <- exp([w]x) R and t <- t + dt, through g with unit weights."""
    sc = mr.refine_scene()
    k0, k1 = mr.cam_of(sc["intrinsics"][0]), mr.cam_of(sc["intrinsics"][1])
    P = sc["rel_pose"].astype(np.float64)
    R, t = P[:3, :3], P[:3, 3] / np.linalg.norm(P[:3, 3])
    xy = sc["xy"].astype(np.float64)[:64]
    big = 1e12                                                    # weights 1 to twelve digits
    sums = mr.pass_sums(xy, k0, k1, R, t, big)

    def res(Rm, tm):
        return mr.residual(mr.sampson(mr.essential(Rm, tm), k0, k1, *(xy[:, i] for i in range(4))))[0]
    eps = 1e-6
    for k in range(6):
        x = np.zeros(6)
        x[k] = eps
        Rp = mr.apply_step(R, t, np.concatenate((x[:3], np.zeros(3))))[0]
        Rm = mr.apply_step(R, t, np.concatenate((-x[:3], np.zeros(3))))[0]
        Jk = (res(Rp, t + x[3:]) - res(Rm, t - x[3:])) / (2 * eps)
        want = (Jk * res(R, t)).sum()
        assert abs(sums[21 + k] - want) <= 1e-6 * (np.abs(Jk * res(R, t)).sum() + 1.0), k


def test_refinement_recovers_the_pose_from_exact_correspondences():
    """Random points at depths 1 - 6, f = 200 px, 256 x 256, coordinates rounded to fp32, started 5 degrees off in rotation and
    17 degrees off in the translation's direction: within 10 iterations both are within 1e-4 degrees of the truth.  (The fp32
    rounding of a coordinate is 1.5e-5 px, about 4e-6 degrees at that focal length: a 25-fold margin.)"""
    sc = mr.refine_scene()
    start = mr.pose_errors(sc["rel_pose"], sc)
    assert abs(start[0] - 5.0) < 1e-3 and abs(start[1] - 17.0) < 1e-3
    pose, stats, _ = mr.refine_pose(sc["xy"], len(sc["xy"]), sc["intrinsics"], sc["rel_pose"], 10, 2.0)
    got = mr.pose_errors(pose, sc)
    print("exact correspondences:", start, "->", got, "stats", stats)
    assert got[0] <= 1e-4 and got[1] <= 1e-4
    assert stats[7] == 0 and stats[6] == 10 and stats[3] == len(sc["xy"]) and stats[1] < 1e-6 * stats[0]
    assert abs(stats[4] - 5.0) < 1e-3 and abs(stats[5] - 17.0) < 1e-3             # how far the state moved: back to the truth
    assert abs(np.linalg.norm(pose[:3, 3]) - np.linalg.norm(sc["rel_pose"][:3, 3].astype(np.float64))) < 1e-12     # the length stays
    assert np.abs(pose[:3, :3] @ pose[:3, :3].T - np.eye(3)).max() < 1e-6         # rel_pose's fp32 rotation, turned


def test_refinement_with_noise_and_outliers():
    """30 % uniformly random outliers and 0.5 px noise, seeds fixed: 20 iterations reduce both errors at least tenfold."""
    sc = mr.refine_scene(noise_px=0.5, outliers=0.3)
    start = mr.pose_errors(sc["rel_pose"], sc)
    pose, stats, _ = mr.refine_pose(sc["xy"], len(sc["xy"]), sc["intrinsics"], sc["rel_pose"], 20, 2.0)
    got = mr.pose_errors(pose, sc)
    print("noise and outliers:", start, "->", got, "stats", stats)
    assert got[0] <= start[0] / 10 and got[1] <= start[1] / 10
    assert stats[7] == 0 and 0.5 * len(sc["xy"]) < stats[2] < 0.8 * len(sc["xy"])  # the outliers' weight is gone


def test_a_dropped_jacobian_term_is_caught_by_the_one_step_bound():
    sc = mr.refine_scene()
    args = (sc["xy"], len(sc["xy"]), sc["intrinsics"], sc["rel_pose"], 1, 2.0)
    pose, _, trace = mr.refine_pose(*args)
    len0 = float(np.linalg.norm(sc["rel_pose"][:3, 3].astype(np.float64)))
    d_delta, b_rot, b_tr, cond = mr.refine_step_bound(trace[0], 2.0, len0)
    print("one step: |d delta| <=", d_delta, "rotation entries", b_rot, "translation entries", b_tr, "cond(A)", cond)
    assert b_rot < 1e-5 and cond < 1e6                            # the bound says something
    again, _, _ = mr.refine_pose(*args)
    assert np.array_equal(pose, again)
    bad, _, _ = mr.refine_pose(*args, defect="dropped term")
    assert np.abs(bad - pose)[:3, :3].max() > 100 * (b_rot + mr.U) and np.abs(bad - pose)[:3, 3].max() > 100 * (b_tr + mr.U)


@pytest.mark.parametrize("n", (1, 5))
def test_underdetermined_pairs_stay_finite(n):
    """One match or five cannot fix five degrees of freedom; the damping and the gauge keep the system positive definite, so
    the reference takes its steps and returns a finite pose."""
    sc = mr.refine_scene()
    pose, stats, _ = mr.refine_pose(sc["xy"], n, sc["intrinsics"], sc["rel_pose"], 10, 2.0)
    print(n, "matches:", stats)
    assert np.isfinite(pose).all() and stats[7] in (0.0, 1.0) and stats[3] == n and stats[1] <= stats[0]


def test_nothing_to_do_is_status_two():
    sc = mr.refine_scene()
    P = sc["rel_pose"]
    zero_t, nan_pose = P.copy(), P.copy()
    zero_t[:3, 3] = 0
    nan_pose[1, 1] = np.nan
    for pose_in, count, iters in ((P, 0, 10), (zero_t, 1000, 10), (nan_pose, 1000, 10), (P, 1000, 0)):
        pose, stats, _ = mr.refine_pose(sc["xy"], count, sc["intrinsics"], pose_in, iters, 2.0)
        assert stats[7] == 2 and not stats[:7].any()
        assert np.array_equal(pose, pose_in.astype(np.float64), equal_nan=True)


# ------------------------------------------------------------------------------------------------------------ photo_coords
@pytest.mark.parametrize("Hi,Wi", ((360, 640), (481, 363), (256, 256)))
def test_photo_coords_inverts_fit_intrinsics(Hi, Wi):
    """A 3-D point seen through the photo's own intrinsics lands on x_photo; seen through fit_intrinsics' model intrinsics it
    lands on x_model; photo_coords takes x_model back to x_photo."""
    size = 256
    rng = np.random.default_rng(Hi)
    K_px = np.array([[0.9 * Wi, 0.0, Wi / 2.0 + 3.0], [0.0, 0.95 * Wi, Hi / 2.0 - 2.0], [0.0, 0.0, 1.0]])
    Km = fit_intrinsics(K_px, Hi, Wi, size)[:3, :3]
    X = np.concatenate((rng.uniform(-0.4, 0.4, size=(50, 2)), np.ones((50, 1))), 1)
    photo, model = (X @ K_px.T)[:, :2], (X @ Km.T)[:, :2]
    xy = np.concatenate((model, model[::-1]), 1)
    back = mt.photo_coords(xy, Hi, Wi, size)
    assert np.abs(back - np.concatenate((photo, photo[::-1]), 1)).max() < 1e-9
    two = mt.photo_coords(xy, (Hi, 256), (Wi, 256), size)          # the second photo is already a model-sized square
    assert np.abs(two[:, :2] - photo).max() < 1e-9 and np.array_equal(two[:, 2:], xy[:, 2:])
    with pytest.raises(ValueError):
        mt.photo_coords(xy[:, :3], Hi, Wi, size)


def test_entry_checks_refuse_host_tensors_and_bad_shapes():
    f = torch.zeros(1, 2, 8, 8)
    with pytest.raises(RuntimeError, match="HIP device only"):
        mt.match_fields((f, f), torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 4), S=32)
    with pytest.raises(RuntimeError, match="HIP device only"):
        mt.refine_pose(mt.Matches(torch.zeros(1, 4, 4), torch.zeros(1, 4, 2), torch.zeros(1, dtype=torch.int32)),
                       torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 4))
    with pytest.raises(ValueError):
        mt.select({"cycle": f, "epi": f, "inside": f, "q": f}, stride=0)
