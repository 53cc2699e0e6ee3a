"""The log's drawings on the MI355X (`pytest -m gpu`): the three kernels of csrc/epipolar.hip against the forms of
tests/epipolar_ref.py, and the two switches of image_summaries / SummaryLog.

Bars (every one is derived in tests/epipolar_ref.py or stated by the rule itself, none comes from a run):
  F, lines       |kernel - numpy float64| <= EPS64 = 64 x 2^-53 relative to the absolute-value products G and G (x, y, 1)
  ends, valid    equal: tests/test_epipolar_ref.py asserts for every case used here that each end point lies further from an
                 integer than the two sides' roundings can move it
  coverage       the set of drawn pixels equals the integer rule exactly while the end points stay within 2^15; in the steep
                 case (2^16 < |y| < 2^20) equal outside the fringe, which that test caps at 16 pixels per line
  values         fl32(0.4 colour + 0.6 v) on a line, the colour on a disc, to 2 ulp of 255; every other pixel has v's bits
  contour        exact
"""
import functools

import numpy as np
import pytest
import torch

from tests import epipolar_ref as er
from tests import summaries_ref as sr
from tests.helpers import to_device

pytestmark = pytest.mark.gpu

ULP255 = float(np.spacing(np.float32(255.0)))
SHAPES = ((3, 32), (1, 48))                                # panel widths 64 and 96: whole 32 x 8 tiles; S = 36 has its own test


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


# --------------------------------------------------------------------------------------------------------------- lines
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("S", [32, 48])
def test_lines_against_float64(dev, B, S):
    from coponerf_amd.summaries import epipolar_lines
    for name in er.CASES:
        _, K, rel, gt, points = er.case(name, B, S)
        ref = er.case_lines(name, B, S)
        args = (K.to(dev), rel.to(dev), gt.to(dev), points.to(dev), S)
        F, lines, ends, valid = epipolar_lines(*args)
        P = len(points)
        assert F.shape == (2, B, 3, 3) and lines.shape == (2, B, P, 3) and ends.shape == (2, B, P, 4) and valid.shape == (2, B, P)
        assert F.dtype == lines.dtype == torch.float64 and ends.dtype == torch.int32 and valid.dtype == torch.uint8
        F, lines, ends, valid = (t.cpu().numpy() for t in (F, lines, ends, valid))
        finite = np.isfinite(ref["F"])                     # a NaN pose: only the entries that are finite upstream are compared
        with np.errstate(invalid="ignore"):
            eF = np.where(finite, np.abs(F - ref["F"]) - er.EPS64 * ref["G"], 0.0)
            eL = np.where(np.isfinite(ref["lines"]), np.abs(lines - ref["lines"]) - er.EPS64 * ref["scale"], 0.0)
            relF = np.nanmax(np.where(finite & (ref["G"] > 0), np.abs(F - ref["F"]) / ref["G"], 0.0))
        print(name, "largest |dF| / G =", relF, "allowed", er.EPS64)
        assert float(eF.max()) <= 0 and float(eL.max()) <= 0, name
        assert np.array_equal(valid.astype(bool), ref["valid"]), name
        assert np.array_equal(ends.astype(np.int64), ref["ends"]), name
        again = epipolar_lines(*args)
        assert all(np.array_equal(a.cpu().numpy(), b, equal_nan=True) for a, b in zip(again, (F, lines, ends, valid))), name


def test_F_against_the_reference_fixture(dev):
    """The kernel's F on the inputs of tests/golden/epipolar_F.npz against what the reference's own two_view_geometry returned."""
    import os
    from coponerf_amd.summaries import default_points, epipolar_lines
    gold = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "epipolar_F.npz")))
    K, rel, gt = er.golden_inputs()
    points = torch.tensor(default_points(er.GOLDEN_SIDE), dtype=torch.int32)
    F = epipolar_lines(K.to(dev), rel.to(dev), gt.to(dev), points.to(dev), er.GOLDEN_SIDE)[0].cpu().numpy()
    G = er.geometry_scale(K, rel, gt)
    for k, name in enumerate(("F", "F_gt")):
        print(name, "largest |dF| / G =", float((np.abs(F[k] - gold[name])[G[k] > 0] / G[k][G[k] > 0]).max()), "allowed", er.EPS64)
        assert float((np.abs(F[k] - gold[name]) - er.EPS64 * G[k]).max()) <= 0, name


# -------------------------------------------------------------------------------------------------------------- panels
@functools.lru_cache(maxsize=None)
def _want(name, B, S, radius, thickness):
    rgb, _, _, _, points = er.case(name, B, S)
    ref = er.case_lines(name, B, S)
    return er.panels(rgb, points.tolist(), er.colors_for(len(points)), ref["ends"], ref["valid"], radius, thickness)


def _run(dev, name, B, S, radius, thickness):
    from coponerf_amd.summaries import epipolar_panels
    rgb, K, rel, gt, points = er.case(name, B, S)
    colors = torch.from_numpy(er.colors_for(len(points)))
    pred, gt_panel = epipolar_panels(rgb.to(dev), K.to(dev), rel.to(dev), gt.to(dev), points.to(dev), colors.to(dev), radius, thickness)
    assert pred.shape == gt_panel.shape == (B, S, 2 * S, 3) and pred.dtype == gt_panel.dtype == torch.float32
    return pred, gt_panel


def _check(dev, name, B, S, radius, thickness):
    rgb = er.case(name, B, S)[0]
    pred, gt_panel = _run(dev, name, B, S, radius, thickness)
    got = torch.stack((pred, gt_panel)).cpu().numpy()
    want, hit, delicate = _want(name, B, S, radius, thickness)
    assert np.isfinite(got).all(), name
    drawn = er.covered(got, rgb)
    lines_drawn = int(er.case_lines(name, B, S)["valid"].sum())
    print(name, (B, S, radius, thickness), "drawn pixels", int(drawn.sum()), "expected", int((hit >= 0).sum()), "fringe", int(delicate.sum()))
    if name == "steep":
        assert int(delicate.sum()) <= 16 * lines_drawn
    else:
        delicate = np.zeros_like(delicate)                 # the exact path: fringe pixels are decided too
    assert np.array_equal(drawn[~delicate], (hit >= 0)[~delicate]), name
    assert np.array_equal(got[(hit < 0) & ~delicate], want[(hit < 0) & ~delicate]), name       # untouched: the view's bits
    worst = float(np.abs(got.astype(np.float64) - want)[~delicate].max())
    print(name, "largest value difference", worst, "allowed", 2 * ULP255)
    assert worst <= 2 * ULP255, name
    again = _run(dev, name, B, S, radius, thickness)
    assert torch.equal(again[0], pred) and torch.equal(again[1], gt_panel)                   # bit-reproducible
    return pred, gt_panel, hit


@pytest.mark.parametrize("B,S", SHAPES)
@pytest.mark.parametrize("radius,thickness", [(2, 3), (5, 10)])
@pytest.mark.parametrize("name", ["generic", "steep"])
def test_panels_against_the_integer_rules(dev, name, B, S, radius, thickness):
    pred, gt_panel, hit = _check(dev, name, B, S, radius, thickness)
    assert name == "steep" or not torch.equal(pred, gt_panel)          # the two steep poses cover the same pixels of so small an image
    assert (hit[..., :S] >= 0).any() and (hit[..., S:] >= 0).any()
    for x, y in ((0, 0), (S - 1, S // 2)) if name == "generic" else ():
        assert hit[0, 0, y, x] >= 9                        # the two clipped discs are there


@pytest.mark.parametrize("name", ["generic", "steep"])
def test_panels_whose_last_tiles_end_outside_the_image(dev, name):
    """S = 36: the panel is 72 = 2.25 tiles wide and 36 = 4.5 tiles high, so the last tile of every row and the last row of tiles
    hold threads beyond the image."""
    _, _, hit = _check(dev, name, 2, 36, 5, 10)
    assert (hit[..., :36] >= 0).any() and (hit[..., 36:] >= 0).any()
    assert (hit[:, :, 32:, :] >= 0).any() and (hit[:, :, :, 64:] >= 0).any()             # something is drawn in the partial tiles


@pytest.mark.parametrize("B,S,radius,thickness", [(3, 32, 5, 10), (1, 48, 2, 3)])
def test_equal_poses_give_equal_panels(dev, B, S, radius, thickness):
    pred, gt_panel, _ = _check(dev, "same", B, S, radius, thickness)
    assert torch.equal(pred, gt_panel)


@pytest.mark.parametrize("B,S,radius,thickness", [(3, 32, 2, 3), (1, 48, 5, 10)])
def test_lines_that_miss_the_image_leave_it_alone(dev, B, S, radius, thickness):
    pred, gt_panel, hit = _check(dev, "miss", B, S, radius, thickness)
    view0 = ((er.case("miss", B, S)[0][:, 0] + 1) * 127.5).to(dev)
    assert not (hit[..., S:] >= 0).any()
    assert torch.equal(pred[:, :, S:], view0) and torch.equal(gt_panel[:, :, S:], view0)


@pytest.mark.parametrize("B,S,radius,thickness", [(3, 32, 5, 10), (1, 48, 2, 3)])
def test_lines_with_b_zero_are_skipped(dev, B, S, radius, thickness):
    from coponerf_amd.summaries import epipolar_lines
    _, K, rel, gt, points = er.case("vertical", B, S)
    F, lines, ends, valid = epipolar_lines(K.to(dev), rel.to(dev), gt.to(dev), points.to(dev), S)
    assert int(valid.sum()) == 0 and int(ends.abs().sum()) == 0 and bool(torch.isfinite(F).all() and torch.isfinite(lines).all())
    pred, gt_panel, hit = _check(dev, "vertical", B, S, radius, thickness)
    view0 = ((er.case("vertical", B, S)[0][:, 0] + 1) * 127.5).to(dev)
    assert torch.equal(pred[:, :, S:], view0) and torch.equal(gt_panel[:, :, S:], view0)
    assert (hit[..., :S] >= 0).any() and bool(torch.isfinite(pred).all())                     # the discs are still drawn


@pytest.mark.parametrize("B,S,radius,thickness", [(3, 32, 5, 10), (1, 48, 2, 3)])
def test_a_nan_pose_costs_its_own_lines_only(dev, B, S, radius, thickness):
    pred, gt_panel, hit = _check(dev, "nan", B, S, radius, thickness)
    clean_pred, clean_gt = _run(dev, "generic", B, S, radius, thickness)
    bad = min(1, B - 1)
    keep = [b for b in range(B) if b != bad]
    assert torch.equal(gt_panel, clean_gt) and torch.equal(pred[keep], clean_pred[keep])
    assert torch.equal(pred[bad, :, S:], clean_pred[bad, :, S:]) is False
    assert not (hit[0, bad, :, S:] >= 0).any() and (hit[0, bad, :, :S] >= 0).any()
    assert bool(torch.isfinite(pred).all())


@pytest.mark.parametrize("B,S,radius,thickness", [(3, 32, 2, 3), (1, 48, 5, 10)])
def test_the_later_of_two_points_on_one_line_wins(dev, B, S, radius, thickness):
    pred, _, hit = _check(dev, "shared", B, S, radius, thickness)
    right = hit[..., S:]
    assert not (right == 0).any() and (right == 2).any() and (right == 1).any()
    colors = er.colors_for(3)
    view0 = (er.case("shared", B, S)[0][:, 0].numpy() + np.float32(1.0)) * np.float32(127.5)
    want = np.float32(0.4) * colors[2] + np.float32(0.6) * view0
    on = right[0] == 2
    assert float(np.abs(pred.cpu().numpy()[:, :, S:][on] - want[on]).max()) <= 2 * ULP255


def test_panels_do_not_depend_on_the_batch(dev):
    from coponerf_amd.summaries import epipolar_panels
    rgb, K, rel, gt, points = er.case("generic", 3, 32)
    colors = torch.from_numpy(er.colors_for(len(points))).to(dev)
    whole = epipolar_panels(rgb.to(dev), K.to(dev), rel.to(dev), gt.to(dev), points.to(dev), colors)
    alone = epipolar_panels(*(t[:1].contiguous().to(dev) for t in (rgb, K, rel, gt)), points.to(dev), colors)
    assert torch.equal(whole[0][:1], alone[0]) and torch.equal(whole[1][:1], alone[1])


def test_default_points_and_colours(dev):
    """No points given: the reference's nine, at the {S/4, S/2, 3S/4}^2 grid, with its colours."""
    from coponerf_amd.summaries import EPIPOLAR_COLORS, default_points, epipolar_panels
    rgb, K, rel, gt, _ = er.case("generic", 1, 48)
    points = torch.tensor(default_points(48), dtype=torch.int32).to(dev)
    colors = torch.tensor(EPIPOLAR_COLORS, dtype=torch.float32).to(dev)
    args = (rgb.to(dev), K.to(dev), rel.to(dev), gt.to(dev))
    given, default = epipolar_panels(*args, points, colors), epipolar_panels(*args)
    assert torch.equal(given[0], default[0]) and torch.equal(given[1], default[1])
    assert default[0][0, 24, 12].tolist() == [222.0, 155.0, 167.0]            # point (12, 24), the second, in its colour
    with pytest.raises(ValueError, match="colors"):
        epipolar_panels(*args, points[:4])
    with pytest.raises(ValueError, match="int32"):
        epipolar_panels(*args, points.long())
    with pytest.raises(ValueError, match="thickness"):
        epipolar_panels(*args, thickness=0)
    with pytest.raises(ValueError, match=r"\(B, 4, 4\)"):
        epipolar_panels(args[0], args[1], args[2][:, :3].contiguous(), args[3])


# ------------------------------------------------------------------------------------------------------------- contour
@pytest.mark.parametrize("S", [8, 36, 40])                # 36: the last tiles end outside the image on both axes
@pytest.mark.parametrize("N", [1, 4])
def test_mask_contour_is_the_border_point_rule(dev, S, N):
    from coponerf_amd.summaries import mask_contour
    masks = list(er.masks(S).items())
    overlay = (torch.arange(N * S * S * 3, dtype=torch.int64) * 37 % 251).to(torch.uint8).reshape(N, S, S, 3)
    for i in range(0, len(masks), 1 if N == 1 else 2):
        names = [masks[(i + j) % len(masks)][0] for j in range(N)]
        mask = np.stack([masks[(i + j) % len(masks)][1] for j in range(N)])
        got = mask_contour(overlay.to(dev), torch.from_numpy(mask).to(dev))
        assert got.dtype == torch.uint8 and got.shape == overlay.shape
        assert np.array_equal(got.cpu().numpy(), er.draw_contour(overlay.numpy(), mask)), names
    loud = torch.from_numpy(masks[2][1] * 255).to(dev)     # any non-zero byte is valid
    assert torch.equal(mask_contour(overlay[:1].to(dev), loud[None]), mask_contour(overlay[:1].to(dev), (loud != 0).to(torch.uint8)[None]))


def test_flow_panels_contour_switch(dev):
    from coponerf_amd.summaries import flow_panels, mask_contour
    rgb, f0, f1, _ = sr.panel_case(2, 32, 4)
    args = (rgb.to(dev), (f0.to(dev), f1.to(dev)))
    plain, off, on = flow_panels(*args), flow_panels(*args, contour=False), flow_panels(*args, contour=True)
    assert all(torch.equal(a, b) for a, b in zip(plain, off))
    assert torch.equal(off[2].cpu(), sr.overlay_rule(off[0].cpu(), off[1].cpu()))             # today's overlay
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])
    assert torch.equal(on[2], mask_contour(off[2], off[1])) and not torch.equal(on[2], off[2])
    assert np.array_equal(on[2].cpu().numpy(), er.draw_contour(off[2].cpu().numpy(), off[1].cpu().numpy()))


# ----------------------------------------------------------------------------------------------------------------- log
@pytest.fixture(scope="module")
def batch(dev):
    model_input, model_output = sr.inputs()
    return to_device(model_input, dev), to_device(model_output, dev)


def test_image_summaries_with_both_switches(dev, batch):
    from coponerf_amd.summaries import EPIPOLAR_TAGS, IMAGE_TAGS, epipolar_panels, image_summaries, make_grid
    model_input, model_output = batch
    S = sr.FIXTURE["S"]
    plain = image_summaries(model_input, model_output, image_shape=(S, S))
    full = image_summaries(model_input, model_output, image_shape=(S, S), epipolar=True, contour=True)
    assert tuple(plain.images) == IMAGE_TAGS and tuple(full.images) == IMAGE_TAGS + EPIPOLAR_TAGS
    assert list(plain.scalars) == list(full.scalars)
    for tag in plain.scalars:
        assert torch.equal(plain.scalars[tag], full.scalars[tag]), tag
    for tag in IMAGE_TAGS:
        if tag.startswith("masked_warped_img"):
            assert full.images[tag].shape == plain.images[tag].shape and not torch.equal(full.images[tag], plain.images[tag])
        else:
            assert torch.equal(full.images[tag], plain.images[tag]), tag
    pred, gt = epipolar_panels(model_input["context"]["rgb"], model_input["context"]["intrinsics"], model_output["rel_pose"],
                               model_output["gt_rel_pose"])
    assert pred.shape == (2, S, 2 * S, 3) and not torch.equal(pred, gt)
    assert torch.equal(full.images["epipolar_pred"], make_grid(pred.permute(0, 3, 1, 2)))
    assert torch.equal(full.images["epipolar_GT"], make_grid(gt.permute(0, 3, 1, 2)))
    assert full.images["epipolar_GT"].shape == (3, S + 4, 2 * (2 * S + 2) + 2)
    only = image_summaries(model_input, model_output, image_shape=(S, S), contour=True)
    assert tuple(only.images) == IMAGE_TAGS and torch.equal(only.images["masked_warped_img"], full.images["masked_warped_img"])


def test_summary_log_switches_add_no_host_read(dev, batch):
    from coponerf_amd.summaries import EPIPOLAR_TAGS, IMAGE_TAGS, SummaryLog, image_summaries
    model_input, model_output = batch
    S = sr.FIXTURE["S"]
    image_summaries(model_input, model_output, image_shape=(S, S), epipolar=True, contour=True)   # first call: the settings' upload
    writer = FakeWriter()
    log = SummaryLog(writer, prefix="val_", lag=1, epipolar=True, contour=True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        log.add(model_input, model_output, 0, image_shape=(S, S))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert log.host_reads == 0 and len(log) == 1 and not writer.images
    log.flush()
    assert log.host_reads == 1
    assert [t for t, _, _ in writer.images] == ["val_" + t for t in IMAGE_TAGS + EPIPOLAR_TAGS] and len(writer.images) == 10
    want = image_summaries(model_input, model_output, image_shape=(S, S), epipolar=True, contour=True)
    for tag, _, img in writer.images:
        assert np.array_equal(img, want.images[tag[4:]].cpu().numpy()), tag

    default = SummaryLog(FakeWriter(), lag=0)
    default.add(model_input, model_output, 3, image_shape=(S, S))
    assert [t for t, _, _ in default.writer.images] == list(IMAGE_TAGS)
