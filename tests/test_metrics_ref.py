"""tests/metrics_ref.py, the float64 yardstick of the evaluation metrics, pinned on the CPU: its filter against the one library
call skimage's SSIM makes, its conventions against torch's, and its fp32 form against the bars the GPU test sets."""
import math
import warnings

import numpy as np
import pytest
import torch

from tests import metrics_ref as mr

SSIM_BAR = 5e-5             # half a unit of the fourth decimal the evaluation prints
SSIM_CEILING = 1e-4         # one unit of that decimal: what fp32 itself may cost on the cancellation cases before their bar
                            # (twice that cost) stops saying anything about the printed figure


@pytest.mark.parametrize("H,W", [(11, 11), (12, 37), (64, 48)])
def test_filter_equals_scipy_gaussian_filter(H, W):
    ndi = pytest.importorskip("scipy.ndimage")
    img = np.random.default_rng(H * 100 + W).uniform(0, 1, (H, W))
    want = ndi.gaussian_filter(img, sigma=1.5, truncate=3.5, mode="reflect")
    got = mr.filter2d(img)
    err = float(np.abs(got - want).max())
    print(f"{H}x{W}: max |filter2d - gaussian_filter| = {err:.2e}")
    assert err <= 1e-14


def test_reflect_index_is_scipys_reflect():
    assert mr.reflect_index(np.arange(-5, 16), 11).tolist() == [4, 3, 2, 1, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 10, 9, 8, 7, 6]
    assert abs(mr.window64().sum() - 1.0) <= 1e-15 and len(mr.window64()) == 11


def test_identical_images_give_one_and_infinity():
    pred, target = mr.make_case("identical", 2, 12, 37)
    assert mr.ssim64(pred, target).tolist() == [1.0, 1.0]
    assert mr.ssim32_straight(pred, target).tolist() == [1.0, 1.0]
    mse = mr.mse64(pred, target)
    assert mse.tolist() == [0.0, 0.0] and np.all(np.isposinf(mr.psnr64(mse)))


def test_only_the_prediction_is_clamped():
    pred, target = mr.make_case("out_of_range", 1, 12, 37)
    assert (np.abs(pred) > 1).mean() > 0.05 and (np.abs(target) > 1).any()
    p, t = mr.to_unit(pred, target)
    assert p.min() >= 0 and p.max() <= 1 and t.max() > 1
    nan = pred.copy()
    nan[0, 3, 4, 1] = np.nan
    assert np.isnan(mr.to_unit(nan, target)[0][0, 3, 4, 1]) and np.isnan(mr.ssim64(nan, target)[0])


def test_bucket_thresholds():
    from coponerf_amd.evaluate import bucket_of
    below = lambda v: math.nextafter(v, 0.0)
    above = lambda v: math.nextafter(v, 1.0)
    for fn in (mr.bucket, bucket_of):
        assert [fn(v) for v in (0.0, below(0.5), 0.5, above(0.5), below(0.75), 0.75, above(0.75), 1.0)] == \
            ["small", "small", "medium", "medium", "medium", "medium", "large", "large"]
    assert bucket_of(float("nan")) is None


@pytest.mark.parametrize("n", [1, 2, 5, 6])
def test_median_and_std_follow_torch(n):
    v = [float(x) for x in np.random.default_rng(n).normal(size=n).astype(np.float32)]
    t = torch.tensor(v, dtype=torch.float64)
    assert v[mr.median_index(v)] == float(t.median())                     # the lower middle for an even count
    if n == 1:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                                # torch says so itself: no degrees of freedom
            assert math.isnan(mr.std(v)) and bool(torch.isnan(t.std()))
    else:
        assert abs(mr.std(v) - float(t.std())) <= 1e-12


def test_summary_ref_bookkeeping():
    rows = [dict(mse=1e-2, psnr=20.0, ssim=0.5, rot=0.1, trans=1.0, angle_trans=0.2, overlap=0.75),
            dict(mse=1e-4, psnr=40.0, ssim=0.9, rot=0.3, trans=3.0, angle_trans=0.4, overlap=0.76),
            dict(mse=1e-3, psnr=30.0, ssim=0.7, rot=0.2, trans=2.0, angle_trans=0.6, overlap=0.1)]
    s = mr.summary_ref(rows, [2, 1])
    assert sorted(s) == ["all", "large", "medium", "small"]
    assert s["all"]["n"] == 2 and s["medium"]["n"] == s["large"]["n"] == s["small"]["n"] == 1
    pooled = (1e-2 + 1e-4) / 2
    assert s["all"]["mse"] == pytest.approx((pooled + 1e-3) / 2, rel=1e-15)
    assert s["all"]["psnr"] == pytest.approx((-10 * math.log10(pooled) + 30.0) / 2, rel=1e-12)   # of the pooled MSE, not 30 dB
    assert s["all"]["rot_median"] == 0.2 and s["all"]["rot_median_at"] == 2 and s["all"]["trans_mean"] == pytest.approx(2.0)
    assert s["all"]["angle_trans_mean"] == pytest.approx((0.3 + 0.6) / 2)
    assert s["medium"]["psnr"] == 20.0 and math.isnan(s["medium"]["rot_std"])


@pytest.mark.parametrize("cid,name,N,H,W", mr.cases(), ids=[c[0] for c in mr.cases()])
def test_straight_fp32_meets_the_bars(cid, name, N, H, W):
    """The bars of tests/test_gpu_metrics.py are ones the reference's own fp32 arithmetic meets on these inputs, the full-size
    case included.  On the flat and bright cases the bar is made of the straight form's own distance, which it cannot miss:
    there the check is the absolute ceiling."""
    pred, target = mr.make_case(name, N, H, W)
    want = mr.ssim64(pred, target)
    d32 = np.abs(mr.ssim32_straight(pred, target) - want)
    dc = np.abs(mr.ssim32_centred(pred, target) - want)
    print(f"{cid}: ssim64 {want.round(6).tolist()}  |straight fp32 - f64| {d32.max():.2e}  |centred fp32 - f64| {dc.max():.2e}")
    assert np.all(np.isfinite(want)) and np.all(want <= 1.0 + 1e-12)
    bar = np.maximum(SSIM_BAR, 2 * d32) if name in ("flat", "bright") else SSIM_BAR
    assert np.all(d32 <= bar)
    if name in ("flat", "bright"):
        assert np.all(d32 <= SSIM_CEILING) and np.all(dc <= SSIM_CEILING)
    if name == "negative_covariance":
        assert np.all(want < 0)
    if name == "identical":
        assert np.all(want == 1.0)
