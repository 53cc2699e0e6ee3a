"""coponerf_amd.summaries on the MI355X (`pytest -m gpu`): the three kernels of csrc/summaries.hip against the float64 forms of
tests/summaries_ref.py, `image_summaries` against the reference's own output (tests/golden/summaries.npz), and the deferred
log.

Bounds (U = 2^-24, the unit roundoff of fp32; every one is derived in tests/summaries_ref.py, none from a run):
  warped values   |kernel - float64 at the kernel's fp32 sampling coordinates| <= WARP_BOUND = 9 U x 255 = 1.4e-4 grey levels:
                  four terms t w with t = (p + 1) * 127.5 <= 255, w = wx wy: 6 roundings per term, weights that sum to 1, and
                  the three additions of the sum.  The coordinates are summaries_ref.coords32's: the kernel's own sequence of
                  single fp32 operations, so they are equal to the last bit and the float64 form picks the kernel's taps.
  masks           equal to float64 on every pixel whose decisions are all at least 1e-3 px from their thresholds; at most
                  0.5 % of the pixels are closer (tests/test_summaries_ref.py holds the reference's own arithmetic to the same).
  overlay         exactly the reference rule on the kernel's own warped values and mask; against the float64 chain, outside
                  the mask band, at most one grey level on at most 1 % of the elements (a warped value within WARP_BOUND of
                  an integer truncates to the other side).
  entropy         |kernel - float64| <= (S + 37) U x mean_rows sum |w log(w + 1e-5)|: summaries_ref.entropy_bound.
  fixture         the fixture's library forms its sampling coordinates with its own roundings, so the end-to-end comparison
                  of warped values allows summaries_ref.fixture_warp_bound: 2 WARP_BOUND + 255 x 4 x coord_bound (0.13 grey
                  levels of 255 at 256 x 256).
"""
import os

import numpy as np
import pytest
import torch

from coponerf_amd import synthetic as syn
from tests import summaries_ref as sr
from tests.helpers import to_device

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "summaries.npz")
ANGLE = 1e-5                                               # radians: the acos bar of tests/test_gpu_metrics.py


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


class FakeWriter:
    def __init__(self):
        self.images, self.scalars = [], []

    def add_image(self, tag, img, step):
        assert isinstance(img, np.ndarray) and img.ndim == 3 and img.shape[0] == 3 and img.dtype == np.float32, (tag, type(img))
        self.images.append((tag, step, img))

    def add_scalar(self, tag, value, step):
        assert isinstance(value, float), (tag, type(value))
        self.scalars.append((tag, step, value))

    def steps(self):
        return sorted({s for _, s, _ in self.images} | {s for _, s, _ in self.scalars})


# --------------------------------------------------------------------------------------------------------- flow panels
@pytest.mark.parametrize("B,S,s", sr.PANEL_CASES)
def test_flow_panels_against_float64(dev, B, S, s):
    from coponerf_amd.summaries import flow_panels
    rgb, f0, f1, ref = sr.panel_case(B, S, s)
    args = (rgb.to(dev), (f0.to(dev), f1.to(dev)))
    warped, mask, overlay = flow_panels(*args)
    assert warped.shape == (2, B, S, S, 3) and mask.shape == (2, B, S, S) and overlay.shape == (2, B, S, S, 3)
    assert warped.dtype == torch.float32 and mask.dtype == torch.uint8 and overlay.dtype == torch.uint8
    fig = sr.compare_panels(warped, mask, overlay, ref)
    print(fig, "WARP_BOUND", sr.WARP_BOUND)
    assert fig["band"] <= 0.005
    assert fig["mask_mismatch"] == 0
    assert 0.2 <= fig["true"] <= 0.75 and bool(mask.max() == 1)
    assert fig["warped_err"] <= sr.WARP_BOUND
    assert torch.equal(overlay.cpu(), sr.overlay_rule(warped.cpu(), mask.cpu()))
    assert fig["overlay_max"] <= 1 and fig["overlay_share"] <= 0.01
    again = flow_panels(*args)
    assert all(torch.equal(a, b) for a, b in zip((warped, mask, overlay), again))        # bit-reproducible


def test_flow_panels_at_a_fractional_scale(dev):
    """S / h = 2.5: the same bounds hold where neither the scale nor its reciprocal is a power of two."""
    from coponerf_amd.summaries import flow_panels
    rgb, f0, f1, ref = sr.fractional_case()
    warped, mask, overlay = flow_panels(rgb.to(dev), (f0.to(dev), f1.to(dev)))
    fig = sr.compare_panels(warped, mask, overlay, ref)
    print(fig, "WARP_BOUND", sr.WARP_BOUND)
    assert fig["band"] <= 0.005 and fig["mask_mismatch"] == 0 and 0.05 <= fig["true"] <= 0.95
    assert fig["warped_err"] <= sr.WARP_BOUND
    assert torch.equal(overlay.cpu(), sr.overlay_rule(warped.cpu(), mask.cpu()))
    assert fig["overlay_max"] <= 1 and fig["overlay_share"] <= 0.01


def test_flow_panels_do_not_depend_on_the_batch(dev):
    from coponerf_amd.summaries import flow_panels
    rgb, f0, f1, _ = sr.panel_case(3, 40, 4)
    whole = flow_panels(rgb.to(dev), (f0.to(dev), f1.to(dev)))
    alone = flow_panels(rgb[:1].contiguous().to(dev), (f0[:1].contiguous().to(dev), f1[:1].contiguous().to(dev)))
    for a, b in zip(whole, alone):
        assert torch.equal(a[:, :1], b)


def test_flow_panels_argument_checks(dev):
    from coponerf_amd.summaries import flow_panels
    rgb, f = torch.zeros(1, 2, 8, 8, 3, device=dev), torch.zeros(1, 2, 4, 4, device=dev)
    with pytest.raises(ValueError, match="S >= h"):
        flow_panels(rgb, (torch.zeros(1, 2, 16, 16, device=dev),) * 2)
    with pytest.raises(ValueError, match=r"\(B, 2, S, S, 3\)"):
        flow_panels(torch.zeros(1, 2, 8, 4, 3, device=dev), (f, f))
    with pytest.raises(ValueError, match="fp32"):
        flow_panels(rgb.double(), (f, f))
    with pytest.raises(ValueError, match="contiguous"):
        flow_panels(rgb, (f.transpose(2, 3), f))


# ------------------------------------------------------------------------------------------------------- depth colours
def test_depth_colors_are_the_table_lookup(dev):
    """Exact equality with matplotlib's arithmetic restated in numpy float32 (summaries_ref.jet_lookup) on, one ulp below and
    one ulp above every d with d / 10 * 256 == k, and at the ends of the range."""
    from coponerf_amd.summaries import depth_colors, jet_table
    vals = []
    for k in (1, 2, 3, 7, 64, 100, 128, 200, 254, 255):
        v = np.float32(k / 25.6)
        vals += [v, np.nextafter(v, np.float32(-np.inf)), np.nextafter(v, np.float32(np.inf))]
    ends = [0.0, 10.0, np.nextafter(np.float32(10), np.float32(np.inf)), -0.5, 12.0, np.nan, -0.0, np.inf, -np.inf, 5.0]
    d = np.array(vals + ends, dtype=np.float32).reshape(5, -1)
    got = depth_colors(torch.from_numpy(d).to(dev))
    assert got.shape == (5, d.shape[1], 3) and got.dtype == torch.float32
    got = got.cpu().numpy()
    assert np.array_equal(got, sr.jet_lookup(d).astype(np.float32))
    table = jet_table().astype(np.float32)
    zero = np.zeros(3, dtype=np.float32)
    want_ends = [table[0], table[255], table[255], table[0], table[255], zero, table[0], table[255], table[0], table[128]]
    assert np.array_equal(got.reshape(-1, 3)[len(vals):], np.stack(want_ends))
    assert np.array_equal(depth_colors(torch.from_numpy(d).to(dev)).cpu().numpy(), got)


# ------------------------------------------------------------------------------------------------------------- entropy
@pytest.mark.parametrize("rows,S", sr.ENTROPY_SHAPES)
def test_attention_entropy_against_float64(dev, rows, S):
    from coponerf_amd.summaries import attention_entropy
    for name, w in sr.entropy_cases(rows, S).items():
        wd = w.to(dev)
        for flag in (False, True):
            first = attention_entropy(wd, nan_to_zero=flag)
            assert first.is_cuda and first.dim() == 0 and first.dtype == torch.float32
            got, want = float(first), float(sr.entropy64(w, flag))
            if name == "nanrow" and not flag:
                assert got != got and want != want
                continue
            print(name, flag, got, want, abs(got - want), sr.entropy_bound(w))
            assert abs(got - want) <= sr.entropy_bound(w), (name, flag)
            assert torch.equal(first, attention_entropy(wd, nan_to_zero=flag))                 # bit-reproducible
            assert torch.equal(first, attention_entropy(wd.view(1, rows, S), nan_to_zero=flag))  # leading dimensions are rows


# ---------------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def batch(dev):
    model_input, model_output = sr.inputs()
    return to_device(model_input, dev), to_device(model_output, dev)


def _grid_samples(grid, tag, shape):
    """The grid's values at the fixture's sample positions of the (N, C, H, W) image it was made of."""
    N, C, H, W = shape
    n, c, y, x = np.unravel_index(sr.positions(tag, N * C * H * W), shape)
    col, row = n % 8, n // 8
    return grid.cpu().numpy()[c, row * (H + 2) + 2 + y, col * (W + 2) + 2 + x].astype(np.float64), n


def test_image_summaries_against_the_reference_fixture(dev, batch):
    from coponerf_amd.summaries import image_summaries
    gold = dict(np.load(GOLDEN))
    model_input, model_output = batch
    S = sr.FIXTURE["S"]
    summary = image_summaries(model_input, model_output, image_shape=(S, S))
    assert set(summary.images) == {k[:-6] for k in gold if k.endswith("_shape")}
    assert set(summary.scalars) == {k[7:] for k in gold if k.startswith("scalar_")}
    assert all(t.is_cuda and t.dtype == torch.float32 for t in list(summary.images.values()) + list(summary.scalars.values()))

    cpu_out = sr.inputs()[1]
    for tag, value in summary.scalars.items():
        got, want = float(value), float(gold["scalar_" + tag])
        if tag == "ent":                                   # both fp32 forms lie within the bound of float64
            tol = 2 * sr.entropy_bound(cpu_out["at_wt"])
        elif tag.startswith("rot_distance"):               # acos at 0.1 - 0.2 rad amplifies one ulp of the cosine 10 x
            tol = ANGLE * (180 / np.pi if "degrees" in tag else 1.0)
        else:
            tol = 1e-6 * abs(want)
        print(tag, got, want, abs(got - want), tol)
        assert abs(got - want) <= tol, tag

    flows = cpu_out["flow"]
    warp_tol = sr.fixture_warp_bound(flows, S)
    print("fixture_warp_bound", warp_tol, "coord_bound", sr.coord_bound(flows, S))
    for tag, grid in summary.images.items():
        shape = tuple(int(v) for v in gold[tag + "_shape"])
        N, C, H, W = shape
        assert tuple(grid.shape) == (3, -(-N // 8) * (H + 2) + 2, min(8, N) * (W + 2) + 2), tag
        got, n = _grid_samples(grid, tag, shape)
        rng = gold[tag + "_range_each"][n].astype(np.float64) if gold[tag + "_flags"][1] else gold[tag + "_range"].astype(np.float64)[None]
        lo, hi = rng[:, 0], rng[:, 1]
        want = (gold[tag + "_values"].astype(np.float64) - lo) / (hi - lo + 1e-5)
        err = np.abs(got - want)
        span = float((hi - lo).min())
        if tag.startswith("warped_img"):                   # the value, the minimum and the maximum may each be off by the bound
            tol = 3 * warp_tol / span + 4 * sr.U
            print(tag, "largest error", err.max(), "allowed", tol)
            assert err.max() <= tol, tag
        elif tag.startswith("masked_warped_img"):
            # bytes: one grey level where a warped value truncates to the other side (value, minimum, maximum: 3 levels after
            # the normalisation), anything inside the mask band (<= 0.5 % of the pixels), and at most 1 % + 0.5 % differ at all
            off, far = float((err > 4 * sr.U).mean()), float((err > 3 / span + 4 * sr.U).mean())
            print(tag, "differing", off, "beyond one level", far)
            assert off <= 0.015 and far <= 0.005, tag
        else:
            print(tag, "largest error", err.max())
            assert err.max() <= 4 * sr.U, tag


# ---------------------------------------------------------------------------------------------------------- host reads
def test_summaries_and_add_read_nothing_on_the_host(dev, batch):
    """As tests/test_gpu_evaluate.py asks of Evaluator.add: with torch's sync debug mode on `error`, any blocking device -> host
    read or pageable copy raises."""
    from coponerf_amd.summaries import SummaryLog, image_summaries
    model_input, model_output = batch
    S = sr.FIXTURE["S"]
    writer = FakeWriter()
    image_summaries(model_input, model_output, image_shape=(S, S))          # first call: the colour table's upload
    log = SummaryLog(writer, prefix="val_", lag=1)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        image_summaries(model_input, model_output, image_shape=(S, S))
        log.add(model_input, model_output, 0, image_shape=(S, S))           # nothing pending: writes nothing
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert log.host_reads == 0 and len(log) == 1 and not writer.images and not writer.scalars
    for k in (1, 2):
        log.add(model_input, model_output, k)                               # square when not told
        assert log.host_reads == k and writer.steps() == list(range(k)) and len(log) == 1
    log.flush()
    assert log.host_reads == 3 and writer.steps() == [0, 1, 2] and len(log) == 0
    log.flush()
    assert log.host_reads == 3
    summary = image_summaries(model_input, model_output, image_shape=(S, S))
    assert [t for t, s, _ in writer.images if s == 1] == ["val_" + t for t in summary.images]
    assert [t for t, s, _ in writer.scalars if s == 1] == ["val_" + t for t in summary.scalars]
    for tag, step, img in writer.images:
        assert np.array_equal(img, summary.images[tag[4:]].cpu().numpy()), (tag, step)
    for tag, step, value in writer.scalars:
        assert value == float(summary.scalars[tag[4:]]), (tag, step)

    later = SummaryLog(FakeWriter(), lag=2)
    for k in range(4):
        later.add(model_input, model_output, k)
        assert later.host_reads == max(0, k - 1) and later.writer.steps() == list(range(max(0, k - 1)))
    now = SummaryLog(FakeWriter(), lag=0)
    now.add(model_input, model_output, 7)
    assert now.host_reads == 1 and now.writer.steps() == [7] and len(now) == 0


def test_evaluator_run_logs_every_batch(dev):
    """Two batches of one 256 x 256 pair (the side get_z is built for) through Evaluator.run with and without a log."""
    from coponerf_amd import CoPoNeRF
    from coponerf_amd.evaluate import Evaluator
    from coponerf_amd.summaries import IMAGE_TAGS, SummaryLog
    model = CoPoNeRF.CoPoNeRF(n_view=2)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(syn.make_full_weights(shapes), strict=True)
    model = model.to(dev).eval()
    loader = []
    for i in range(2):
        inp = syn.make_inputs(1, 256, 256, 0, seed=170 + i, full_image=True)
        loader.append((inp, {"rgb": inp["query"]["rgb"]}, [0.4 + 0.3 * i]))
    writer = FakeWriter()
    log = SummaryLog(writer, lag=1)
    ev = Evaluator().run(model, loader, summary_log=log)
    assert ev.host_reads == 0 and log.host_reads == 1 and writer.steps() == [0]
    log.flush()
    assert log.host_reads == 2 and writer.steps() == [0, 1]
    for step in (0, 1):
        assert sorted(t for t, s, _ in writer.images if s == step) == sorted(IMAGE_TAGS)
        scalars = {t: v for t, s, v in writer.scalars if s == step}
        assert "ent" in scalars and all(np.isfinite(v) for t, v in scalars.items() if t != "rot_distance_degrees_std"), scalars
        assert scalars["rot_distance_degrees_std"] != scalars["rot_distance_degrees_std"]        # one pose: torch.std is NaN
    plain = Evaluator().run(model, loader)
    assert torch.equal(ev.rows(), plain.rows())
