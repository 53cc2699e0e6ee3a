"""tests/pose_eval_ref.py pinned on the CPU: the restatement of cpn_pose_errors and cpn_residual_stats (round 25) against
independent numpy formulas, the conditions on the GPU fixtures that allow tests/test_gpu_pose_eval.py to compare bits, the AUC of
coponerf_amd.evaluate.pose_auc, and seeded defects that must each fail an assertion."""
import math

import numpy as np
import pytest

from coponerf_amd import _hip
from coponerf_amd.evaluate import pose_auc
from tests import matches_ref as mr
from tests import pose_eval_ref as pe

E = 2.0 ** -53


def test_header_declares_the_entry_points():
    """Two additive symbols and the limit of P, Q and T; the ABI version stays."""
    assert _hip.CONSTANTS["POSE_EVAL_MAX"] == 8 and _hip.ABI_VERSION == 12
    assert len(_hip.SIGNATURES["cpn_pose_errors"]) == 6 and len(_hip.SIGNATURES["cpn_residual_stats"]) == 17


def _partition(values, k):
    return np.partition(np.abs(np.asarray(values, dtype=np.float64)), k)[k]


def _value_sets():
    rng = np.random.default_rng(7)
    sets = {name: v.astype(np.float64) / np.sqrt(2.0) for name, v in pe.residual_sets().items()}
    sets["uniform"] = rng.uniform(0.0, 3.0, 1000)
    sets["spread"] = 10.0 ** rng.uniform(-12.0, 3.0, 4096)           # float64 mantissas: the low digits differ too
    sets["one"] = np.array([0.7])
    return sets


# -------------------------------------------------------------------------------------------------------------- quantiles
@pytest.mark.parametrize("name", ["zero", "tied", "wide", "random", "uniform", "spread", "one"])
def test_radix_descent_is_the_order_statistic(name):
    """radix_select, the kernel's descent, returns np.partition's element at every rank tried - in its bits - on random, tied,
    all-zero and wide-range values; -0 and +0 are one key and come back as +0."""
    v = _value_sets()[name]
    n = len(v)
    for k in sorted({0, 1 % n, (n - 1) // 2, n // 2, int(0.9 * (n - 1)), n - 1}):
        got, want = pe.radix_select(v, k), _partition(v, k)
        assert got.view(np.uint64) == np.float64(want).view(np.uint64), (name, k, got, want)
        assert not np.signbit(got)
    if name == "spread":                                            # every one of the eight digits takes more than one value
        keys = pe.keys_of(v)
        assert all(len(np.unique((keys >> np.uint64(56 - 8 * p)) & np.uint64(255))) > 1 for p in range(8))


def test_zero_residuals_are_one_key():
    """Exact matches give r = +-0: both signs are in the fixture, their keys are equal, and every statistic of the set is +0."""
    xy, counts, K, poses = pe.shear_case()
    a, ok = pe.abs_residuals(xy[0], counts[0], K[0], poses[0, 0])
    with np.errstate(all="ignore"):
        s = mr.sampson(mr.essential(np.eye(3), np.array([-1.0, 0.0, 0.0])), mr.cam_of(K[0, 0]), mr.cam_of(K[0, 1]),
                       *(xy[0, :300, i].astype(np.float64) for i in range(4)))
        r, _ = mr.residual(s)
    assert ok.all() and np.signbit(r).any() and not np.signbit(r).all() and not r.any()
    assert (pe.keys_of(r) == 0).all()
    w = pe.want_stats("shear")[0]
    assert w["usable"][0] == 300 and not w["quant"][0].any() and not np.signbit(w["quant"][0]).any()
    assert list(w["within"][0]) == [300, 300] and w["sigma"][0, 0] == 0.0 and w["sigma"][0, 1] == 0.0


def test_shear_rows_give_their_residuals():
    """The construction of the shear fixtures: |r| is |v| / sqrt(2) in the residual's own operations, so the wide set spans
    1e-12 .. 1e3 px."""
    xy, counts, K, poses = pe.shear_case()
    a, ok = pe.abs_residuals(xy[2], counts[2], K[2], poses[2, 0])
    v = np.abs(pe.residual_sets()["wide"].astype(np.float64))
    assert ok.all() and np.array_equal(a, v / np.sqrt(2.0))
    assert a.min() < 1e-11 and a.max() > 1e2


@pytest.mark.parametrize("case", ["scene", "shear"])
def test_restatement_against_partition(case):
    """residual_stats' quant, within and sigmas from independent numpy: np.partition over the usable |r|, counts by comparison,
    the sigma formulas with np.sum (block_sum's order differs from it by rounding only: n 2^-53 relative)."""
    xy, counts, K, poses = pe.scene_case() if case == "scene" else pe.shear_case()
    for b, w in enumerate(pe.want_stats(case)):
        for p in range(poses.shape[1]):
            if w["status"][p]:
                assert w["usable"][p] == 0 and np.isnan(w["quant"][p]).all() and not w["within"][p].any() and np.isnan(w["sigma"][p]).all()
                continue
            a, ok = pe.abs_residuals(xy[b], counts[b], K[b], poses[b, p])
            u = a[ok]
            assert w["usable"][p] == len(u) > 0
            for j, q in enumerate(pe.Q_GPU):
                k = int(math.floor(q * (len(u) - 1)))
                assert w["quant"][p, j] == np.partition(u, k)[k]
                assert pe.radix_select(u, k) == w["quant"][p, j]
            assert w["quant"][p, 0] == u.min() and w["quant"][p, 3] == u.max()
            assert w["quant"][p, 1] == np.sort(u)[(len(u) - 1) // 2]          # torch.median's lower middle
            assert list(w["within"][p]) == [int((u <= t).sum()) for t in pe.THR_GPU]
            if len(u) > 5:
                s0 = 1.4826 * (1.0 + 5.0 / (len(u) - 5)) * np.sort(u)[(len(u) - 1) // 2]
                assert abs(w["sigma"][p, 0] - s0) <= 4 * E * s0
                inl = u[u <= 2.5 * w["sigma"][p, 0]]
                if len(inl) > 5:
                    s1 = math.sqrt(np.sum(inl * inl) / (len(inl) - 5))
                    assert abs(w["sigma"][p, 1] - s1) <= (len(u) + 4) * E * s1
                else:
                    assert np.isnan(w["sigma"][p, 1])
            else:
                assert np.isnan(w["sigma"][p]).all()


def test_few_rows_and_statuses():
    """Counts 0, 1, 5 and 6 of the shear batch, and 2 beside them: the stated NaNs and statuses; the pose without a translation
    and the pose with a NaN entry have status 2 whatever the rows."""
    xy, counts, K, poses = pe.shear_case()
    w = pe.want_stats("shear")
    assert list(counts[4:]) == [0, 1, 5, 6]
    assert w[4]["status"][0] == 1 and w[4]["usable"][0] == 0 and np.isnan(w[4]["quant"][0]).all() and np.isnan(w[4]["sigma"][0]).all()
    for b, n in ((5, 1), (6, 5)):
        assert w[b]["status"][0] == 0 and w[b]["usable"][0] == n and np.isfinite(w[b]["quant"][0]).all() and np.isnan(w[b]["sigma"][0]).all()
    assert w[7]["usable"][0] == 6 and np.isfinite(w[7]["sigma"][0, 0])           # 1.4826 (1 + 5 / 1) median
    assert w[7]["sigma"][0, 0] == (1.4826 * 6.0) * w[7]["quant"][0, 1]
    two = pe.residual_stats(xy[2], 2, K[2], poses[2], pe.Q_GPU, pe.THR_GPU)
    assert two["usable"][0] == 2 and two["quant"][0, 1] == two["quant"][0, 0] and np.isnan(two["sigma"][0]).all()
    assert all(x["status"][1] == 2 for x in w) and all(x["status"][2] == 2 for x in pe.want_stats("scene"))
    assert w[3]["usable"][0] == 399                                    # the NaN row inside the count is not usable
    # n_in <= 5: a median of 0 among larger values cuts everything but the zeros
    v = np.array([0.0] * 4 + [1.0, 2.0, 3.0], dtype=np.float32)
    few = pe.residual_stats(pe.shear_rows(v), 7, K[0], poses[0, :1], (0.5,), (1.0,))
    assert few["usable"][0] == 7 and few["sigma"][0, 0] == 0.0 and np.isnan(few["sigma"][0, 1])


@pytest.mark.parametrize("case", ["scene", "shear"])
def test_fixture_margins(case):
    """No usable |r| of a GPU fixture lies within 1e-9 px of a threshold or of the 2.5 sigma[0] cut (a level of exactly 0 apart:
    pose_eval_ref.threshold_margin says why), so the counts and n_in do not hang on the last bits of a residual."""
    xy, counts, K, poses = pe.scene_case() if case == "scene" else pe.shear_case()
    for b in range(len(xy)):
        assert pe.threshold_margin(xy[b], counts[b], K[b], poses[b], pe.THR_GPU) >= pe.MARGIN, b
    if case == "scene":
        w = pe.want_stats(case)
        assert [list(x["usable"]) for x in w] == [[257, 257, 0], [511, 511, 0]]
        assert all(0 < x["within"][p, 1] < x["usable"][p] for x in w for p in (0, 1))     # the threshold divides the matches
        assert all(x["sigma"][0, 1] < x["sigma"][1, 1] for x in w)                        # the truth fits better than 5 degrees off


# ------------------------------------------------------------------------------------------------------------ pose errors
def test_pose_errors_against_acos_in_float64():
    """At 1 .. 179 degrees the atan2 forms agree with acos of the cosine in float64 as far as the fp32 ENTRIES allow: a product of
    two rotations rounded to fp32 is off a rotation by up to 3 x 2^-24 per entry, 2^-21 on the trace; the atan2 form passes that on
    as it is, acos of the cosine multiplied by 1 / sin(angle)."""
    gt = np.eye(4)
    gt[:3, :3], gt[:3, 3] = mr.rodrigues((1.0, 0.2, 0.5), 40.0), (-0.5, 0.25, 1.5)
    for deg in (1.0, 10.0, 45.0, 90.0, 135.0, 170.0, 179.0):
        pose = np.eye(4)
        pose[:3, :3] = mr.rodrigues((0.3, 1.0, -0.2), deg) @ gt[:3, :3]
        pose[:3, 3] = mr.rodrigues(np.cross(gt[:3, 3], (0.0, 0.0, 1.0)), deg) @ gt[:3, 3] * 1.7
        p32, g32 = pose.astype(np.float32)[None], gt.astype(np.float32)
        got, want = pe.pose_errors(p32, g32)[0], pe.acos_rule64(p32, g32)[0]
        assert abs(np.degrees(got[0]) - deg) < 1e-4 and abs(np.degrees(got[2]) - deg) < 1e-4          # fp32 inputs
        tol = 2.0 ** -21 * (1.0 + 1.0 / math.sin(math.radians(deg)))
        assert abs(got[0] - want[0]) <= tol and abs(got[2] - want[2]) <= tol, (deg, got, want)
        assert abs(got[1] - want[1]) <= 8 * E * want[1]


def test_small_and_near_pi_rotations_resolve_where_fp32_acos_cannot():
    """Rodrigues rotations of 1e-6, 0.03 and 179.9999 degrees in fp32 entries: the float64 atan2 form is within 2^-22 of the
    angle (the entries' own rounding), the reference's fp32 rule is off by its quantisation: below 1 fp32 steps by 2^-24, so the
    angle comes in steps of sqrt(2 k 2^-24) rad = 0.020, 0.028, .. degrees - the reason for the rot64 columns."""
    poses, gt = pe.errors_case()
    got, ref32 = pe.pose_errors(poses[0], gt[0])[:, 0], pe.acos_rule32(poses[0], gt[0]).astype(np.float64)
    for p, deg in enumerate(pe.ANGLES_DEG):
        true = math.radians(deg)
        assert abs(got[p] - true) <= 2.0 ** -22 * true, (deg, got[p])
    assert ref32[0] == 0.0                                              # 1e-6 degrees: nothing left
    assert abs(ref32[1] - math.radians(0.03)) > 1e-5                    # 0.03 degrees lies between two steps
    assert abs(ref32[4] - math.radians(179.9999)) > 1e-6                # the cosine is -1 in fp32
    assert abs(ref32[3] - math.radians(90.0)) < 1e-6                    # where acos is well conditioned fp32 is fine
    with_gt = pe.pose_errors(poses[1], gt[1])[:, 0]                     # a product of two rounded matrices: 1e-7 rad of noise
    assert all(abs(with_gt[p] - math.radians(d)) < 5e-7 for p, d in enumerate(pe.ANGLES_DEG))


def test_direction_angle_and_nans():
    poses, gt = pe.errors_case()
    e0, e2 = pe.pose_errors(poses[0], gt[0]), pe.pose_errors(poses[2], gt[2])
    assert e0[0, 2] == 0.0 and abs(e0[1, 2] - math.pi) < 1e-6 and abs(e0[2, 2] - math.pi / 2) < 1e-6
    assert abs(e0[3, 2] - math.radians(1e-5)) < 2e-8                    # fp32 entries; acos would return 0 or 3e-4
    assert np.isnan(e0[4, 2]) and np.isfinite(e0[4, :2]).all()          # a zero translation: the direction alone
    assert np.isnan(e2[1]).all() and np.isnan(e2[2]).all()              # a NaN and an inf entry: the whole pose, that pose alone
    assert np.isfinite(e2[[0, 3, 4], :2]).all() and np.isnan(e2[[0, 3, 4], 2]).all()          # gt without a translation
    assert pe.ulps(np.array([1.0, np.nan]), np.array([1.0 + 2 * np.spacing(1.0), np.nan])).tolist() == [2.0, 0.0]


# -------------------------------------------------------------------------------------------------------------------- AUC
def test_auc_by_hand_and_by_brute_force():
    # five errors, threshold 5: the curve runs (0, 0) (1, .2) (2, .4) (3, .6) (4, .8) and stays at .8 to 5:
    # area = .1 + .3 + .5 + .7 + .8 = 2.4, over 5
    got = pose_auc([3.0, 1.0, 6.0, 4.0, 2.0], (5, 10, 20))
    assert got[0] == pytest.approx(2.4 / 5, abs=1e-15)
    # threshold 10: .. (4, .8) (6, 1.) and 1. to 10: 2.4 - .8 + (.8 + 1.) + 4 = 7.4... by segments: .1 + .3 + .5 + .7 + 1.8 + 4.
    assert got[1] == pytest.approx(7.4 / 10, abs=1e-15) and got[2] == pytest.approx(17.4 / 20, abs=1e-15)
    assert pose_auc([float("nan")] * 3, (5,)) == [0.0] and pose_auc([0.0, 0.0], (5,)) == [1.0]
    assert pose_auc([1.0, float("nan")], (5,))[0] == pytest.approx((0.25 + 2.0) / 5, abs=1e-15)       # a NaN is a miss
    rng = np.random.default_rng(3)
    errs = np.abs(rng.normal(scale=8.0, size=200))
    errs[::17] = np.nan
    for t, v in zip((5, 10, 20), pose_auc(list(errs), (5, 10, 20))):
        assert abs(v - pe.auc_brute(errs, float(t))) <= 1.0 / 200000 + 1e-12 and 0.0 < v < 1.0


# ---------------------------------------------------------------------------------------------------------- seeded defects
@pytest.mark.parametrize("defect", pe.DEFECTS + ("missing digit",))
def test_seeded_defects_fail(defect):
    """An upper median, a rank over all rows, < for <= and a missing radix digit each change a value the tests above pin."""
    xy, counts, K, poses = pe.shear_case()
    good = pe.want_stats("shear")
    if defect == "missing digit":
        v = _value_sets()["spread"]
        k = len(v) // 2
        assert pe.radix_select(v, k, defect) != _partition(v, k)
        return
    b = {"upper median": 1, "all rows": 3, "strict": 0}[defect]       # the tied set; the NaN row inside the count; zeros at level 0
    bad = pe.residual_stats(xy[b], counts[b], K[b], poses[b], pe.Q_GPU, pe.THR_GPU, defect)
    if defect == "upper median":
        two = pe.residual_stats(pe.shear_rows(np.array([1.0, 2.0], dtype=np.float32)), 2, K[0], poses[0, :1], (0.5,), (1.0,), defect)
        assert two["quant"][0, 0] == 2.0 / np.sqrt(2.0)                 # the lower middle is 1 / sqrt(2)
        ws = pe.residual_stats(xy[7], counts[7], K[7], poses[7], pe.Q_GPU, pe.THR_GPU, defect)
        assert ws["sigma"][0, 0] != good[7]["sigma"][0, 0]
    elif defect == "all rows":
        assert bad["quant"][0, 3] == np.inf != good[b]["quant"][0, 3]
    else:
        assert list(bad["within"][0]) == [0, 300] and np.isnan(bad["sigma"][0, 1]) and good[b]["sigma"][0, 1] == 0.0
