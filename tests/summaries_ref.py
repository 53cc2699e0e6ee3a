"""Yardsticks of the on-device log (coponerf_amd/summaries.py, csrc/summaries.hip) and the inputs of its tests.

  inputs(...)            the synthetic batch of tests/golden/summaries.npz (make_golden_summaries.py): pure functions of seeds
  stock_summaries(...)   an fp32 stock-op restatement of summary/summaries.py:106-235 minus its two OpenCV pieces (the epipolar
                         drawings and the contour of overlay_semantic_mask): every image BEFORE make_grid with the flags the
                         reference passes to it, and every scalar
  coords32(...)          the upsampled flow and the sampling coordinates of `warp` as an explicit sequence of fp32 operations,
                         one rounding each - the sequence csrc/flow_warp.h runs with contraction off
  panels64(...)          float64 flow panels at GIVEN fp32 sampling coordinates, lifted (the device of ssim_ref.ref64_loss: a
                         coordinate within an ulp of an integer picks another tap pair in float64 than in fp32, so a float64
                         run on its own coordinates is no yardstick for an fp32 one), with the distance of every mask decision
                         from its threshold
  overlay_rule(...)      overlay_semantic_mask(color=[255, 102, 51], alpha=0.5) without the contour, in integers
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from coponerf_amd import synthetic as syn
from coponerf_amd.summaries import IMAGE_TAGS, jet_table
from tests import ssim_ref

SEED = 97
FIXTURE = dict(B=2, S=256, s=4)
SAMPLES = 16384
COLOR = (255, 102, 51)
BAND = 1e-3                                                 # px: a mask decision closer than this to a threshold is not compared
PANEL_CASES = ((2, 32, 4), (3, 40, 4), (2, 24, 2), (2, 256, 4))       # (B, S, s) of ssim_ref.case(B, S, S, s)
U = 2.0 ** -24                                              # unit roundoff of fp32

# One warped value is sum_k t_k w_k over four taps with t_k = (p_k + 1) * 127.5 <= 255 and w_k = wx wy.  Roundings on the way
# of one term: wx, wy (a difference each), their product, the two operations of t_k, the product t_k w_k: 6; the weights sum
# to 1, so the four terms together carry 6 U x 255.  The three additions of the sum add U x 255 each at most: 9 U x 255.
WARP_BOUND = 9 * U * 255.0


def coord_bound(flows, S):
    """How far (pixels, per axis) an fp32 sampling coordinate of `warp` may lie from the exact one, from the operation count
    of the two nested forms.  The upsample: source index (2 roundings), its two weights per axis (2), and per value a product
    and a sum along x, a product and a sum along y and the scale (5): 9 roundings relative to max |up|.  utils.warp and
    grid_sample's unnormalisation: v = g + up, / (S - 1), - 1, + 1, * S, - 1 (the factors 2 and / 2 are exact): 6 roundings
    relative to max(|v|, S) S / (S - 1).  A library that contracts some of these into FMAs rounds less often, never more."""
    up = max(float(ssim_ref.upsample(f.double(), S, S).abs().max()) for f in flows)
    return (9 * up + 6 * (S - 1 + up) * S / (S - 1)) * U


def fixture_warp_bound(flows, S):
    """What two fp32 forms of a warped value in [0, 255] may differ by when each forms its own sampling coordinates (the kernel
    with contraction off, the library that wrote the fixture in its own way): zero-padded bilinear interpolation of values in
    [0, 255] moves by at most 255 per pixel of coordinate error and axis, both forms err by coord_bound on both axes, and each
    carries WARP_BOUND of its own."""
    return 2 * WARP_BOUND + 255.0 * 4 * coord_bound(flows, S)


def inputs(B=FIXTURE["B"], S=FIXTURE["S"], s=FIXTURE["s"], seed=SEED):
    """(model_input, model_output) on the CPU: images and flows of ssim_ref.case, a prediction that leaves [-1, 1], depths in
    [-1, 12) with a NaN every 4099 rays, softmax-like attention rows (some exactly 0), poses 0.1 .. 0.3 rad off the rig's."""
    rgb, f0, f1 = ssim_ref.case(B, S, S, s, seed=seed)
    R = S * S
    depth = syn.uniform((B, R, 1), seed, -1.0, 12.0, stream=11)
    depth.view(-1)[::4099] = float("nan")
    w = syn.uniform((2 * B, 96, 64), seed, 0.0, 1.0, stream=12)
    w = torch.where(w < 0.25, torch.zeros_like(w), w)
    at_wt = (w / w.sum(-1, keepdim=True)).contiguous()
    rel, gt_rel = torch.eye(4).repeat(B, 1, 1), torch.eye(4).repeat(B, 1, 1)
    for b in range(B):
        rel[b, :3, :3] = torch.from_numpy(syn._rot_y(-0.2 - 0.1 * b).astype(np.float32))
        rel[b, :3, 3] = torch.tensor([0.3, 0.06 * (b + 1), 0.05 - 0.03 * b])
    gt_rel[:, :3, :3] = torch.from_numpy(syn._rot_y(-0.1).astype(np.float32))
    gt_rel[:, 0, 3] = 0.3
    K = torch.eye(4)
    K[0, 0] = K[1, 1] = 0.8 * S
    K[0, 2] = K[1, 2] = S / 2.0
    model_input = {"context": {"rgb": rgb, "intrinsics": K.repeat(B, 2, 1, 1)},
                   "query": {"rgb": syn.uniform((B, 1, R, 3), seed, -1.0, 1.0, stream=13)}}
    model_output = {"rgb": syn.uniform((B, 1, R, 3), seed, -1.2, 1.2, stream=14), "depth_ray": depth, "at_wt": at_wt,
                    "flow": (f0, f1), "rel_pose": rel, "gt_rel_pose": gt_rel}
    return model_input, model_output


def positions(tag, numel):
    """The seeded sample of element positions the fixture stores values at (flat indices into the (N, C, H, W) image)."""
    return (syn._bits(SAMPLES, SEED, 200 + IMAGE_TAGS.index(tag)) % np.uint64(numel)).astype(np.int64)


# ------------------------------------------------------------------------------------------------ the stock restatement
def jet_lookup(depth):
    """cmap(depth / 10)[..., :3] of a float32 numpy array as matplotlib evaluates it: (..., 3) float64."""
    xa = depth.astype(np.float32) / 10.
    xa = xa * np.float32(256)
    with np.errstate(invalid="ignore"):
        idx = np.where(xa < 0, 0, np.where(xa >= 256, 255, xa.astype(np.int64)))
    out = jet_table()[np.where(np.isnan(xa), 0, idx)]
    out[np.isnan(xa)] = 0.0
    return out


def overlay_rule(warped, mask):
    """summaries.py:42-63 at color=[255, 102, 51], alpha=0.5 without the contour: warped (..., 3) in [0, 255], mask (...) bool ->
    uint8 (..., 3).  0.5 u8 + 0.5 colour is exact in binary floating point, its truncation the integer halving."""
    u = warped.to(torch.uint8).to(torch.int32)
    blend = (u + torch.tensor(COLOR, dtype=torch.int32, device=u.device)) >> 1
    return torch.where(mask.bool().unsqueeze(-1), u, blend).to(torch.uint8)


def entropy(at_wt, nan_to_zero=False):
    """summaries.py:116-117, or wrapper.py:128-130 with nan_to_zero, in at_wt's precision."""
    ent = -(at_wt * torch.log(at_wt + 1e-5)).sum(dim=-1)
    if nan_to_zero:
        ent = torch.where(torch.isnan(ent), torch.zeros_like(ent), ent)
    return ent.mean()


def stock_panels(rgb, f0, f1):
    """summaries.py:163-207 minus the contour in stock ops of rgb's dtype: (warped (2, B, S, S, 3), mask (2, B, S, S) bool,
    overlay (2, B, S, S, 3) uint8, up0)."""
    S = rgb.shape[2]
    up = (ssim_ref.upsample(f0, S, S), ssim_ref.upsample(f1, S, S))
    warped, masks = [], []
    for d in (0, 1):
        cyc = torch.norm(up[d] + ssim_ref.warp(up[1 - d], up[d]), dim=1).le(10)
        m = up[d] + ssim_ref._grid(S, S, up[d])
        inside = m[:, 0].ge(0) & m[:, 0].le(S - 1) & m[:, 1].ge(0) & m[:, 1].le(S - 1)
        masks.append(cyc * inside)
        src = ((rgb[:, 1 - d] + 1) * 127.5).permute(0, 3, 1, 2)
        warped.append(ssim_ref.warp(src, up[d]).permute(0, 2, 3, 1))
    warped, masks = torch.stack(warped), torch.stack(masks)
    return warped, masks, overlay_rule(warped, masks), up[0]


def stock_summaries(model_input, model_output, image_shape):
    """({tag: (image (N, C, H, W) before make_grid, normalize, scale_each)}, {tag: 0-dim tensor}) as the reference forms them."""
    H, W = image_shape
    images, scalars = {}, {}
    predictions = model_output["rgb"].reshape(-1, H, W, 3).permute(0, 3, 1, 2).clamp(-1, 1)
    if "at_wt" in model_output:
        scalars["ent"] = entropy(model_output["at_wt"])
    images["predictions"] = (predictions, True, False)
    depth = jet_lookup(model_output["depth_ray"].reshape(-1, H, W).cpu().numpy()).transpose(0, 3, 1, 2)
    images["depth_images"] = (torch.Tensor(depth), True, True)
    ctx = model_input["context"]["rgb"]
    images["context_images"] = (ctx.flatten(0, 1).permute(0, 3, 1, 2), True, False)
    query = model_input["query"]["rgb"].reshape(-1, H, W, 3).permute(0, 3, 1, 2)
    images["query_images"] = (query, True, False)
    warped, _, overlay, up0 = stock_panels(ctx, model_output["flow"][0], model_output["flow"][1])
    view255 = (ctx + 1) * 127.5
    for d, suffix in ((0, ""), (1, "_flip")):
        panel = torch.cat((view255[:, 1 - d], warped[d], view255[:, d]), dim=-2)
        images["warped_img" + suffix] = (panel.permute(0, 3, 1, 2), True, False)
        images["masked_warped_img" + suffix] = (overlay[d].float().permute(0, 3, 1, 2), True, False)
    scalars["flow_mean"] = up0.flatten(-2, -1).mean(-1)[0, 0]
    scalars["out_min"], scalars["out_max"] = predictions.min(), predictions.max()
    rel, gt_rel = model_output["rel_pose"], model_output["gt_rel_pose"]
    m = torch.bmm(rel[:, :3, :3], gt_rel[:, :3, :3].transpose(1, 2))
    theta = torch.acos(((m[:, 0, 0] + m[:, 1, 1] + m[:, 2, 2] - 1) / 2).clamp(-1, 1))
    scalars["rot_distance"] = theta.mean()
    deg = theta / np.pi * 180
    scalars["rot_distance_degrees_mean"], scalars["rot_distance_degrees_std"] = deg.mean(), deg.std()
    scalars["rot_distance_degrees_max"] = deg.max()
    scalars["tran_L1"] = F.mse_loss(rel[:, :3, 3], gt_rel[:, :3, 3])
    scalars["trgt_min"], scalars["trgt_max"] = query.min(), query.max()
    return images, scalars


# ----------------------------------------------------------------------------------------------- the float64 yardstick
def coords32(flow, S):
    """(up (B, 2, S, S), coords (B, 2, S, S)) fp32: F.interpolate(flow, S, mode="bilinear") * (S / h) and the pixel coordinates
    (ix, iy) `warp` samples at, written out as single fp32 operations in ATen's order (area_pixel_compute_source_index, the
    interpolation along x inside the one along y, utils.warp's normalisation, grid_sample's unnormalisation)."""
    assert flow.dtype == torch.float32
    h = flow.shape[2]
    rs = torch.tensor(h, dtype=torch.float32) / torch.tensor(S, dtype=torch.float32)
    dst = torch.arange(S, dtype=torch.float32)
    src = (rs * (dst + 0.5) - 0.5).clamp(min=0)
    i0 = src.to(torch.int64).clamp(max=h - 1)
    i1 = i0 + (i0 < h - 1).to(torch.int64)
    l1 = src - i0.to(torch.float32)
    l0 = 1.0 - l1
    ya, yb, xa, xb = i0[:, None], i1[:, None], i0[None, :], i1[None, :]
    ly0, ly1, lx0, lx1 = l0[:, None], l1[:, None], l0[None, :], l1[None, :]
    up = (ly0 * (lx0 * flow[:, :, ya, xa] + lx1 * flow[:, :, ya, xb]) + ly1 * (lx0 * flow[:, :, yb, xa] + lx1 * flow[:, :, yb, xb]))
    up = up * torch.tensor(S / h, dtype=torch.float32)
    return up, ssim_ref.unnormalised_coords(up)


def panels64(rgb, f0, f1, coords=None):
    """Float64 flow panels of rgb (B, 2, S, S, 3), f0, f1 (B, 2, h, h) at the fp32 sampling coordinates `coords` = (c0, c1)
    (default: coords32's).  Returns a dict of (2, B, ...) tensors: warped (.., S, S, 3) float64, mask (.., S, S) bool, margin
    (.., S, S): the smallest distance in pixels of the mask's decisions from their thresholds (|norm - 10|, the mapping's
    distance from 0 and from S - 1 on both axes)."""
    S = rgb.shape[2]
    fl = (f0, f1)
    if coords is None:
        coords = tuple(coords32(f, S)[1] for f in fl)
    up = tuple(ssim_ref.upsample(f.double(), S, S) for f in fl)
    warped, masks, margins = [], [], []
    for d in (0, 1):
        ix, iy = coords[d][:, 0].double(), coords[d][:, 1].double()
        err = up[d] + ssim_ref.sample_taps(up[1 - d], ix, iy)
        norm = torch.sqrt(err[:, 0] ** 2 + err[:, 1] ** 2)
        m = up[d] + ssim_ref._grid(S, S, up[d])
        inside = m[:, 0].ge(0) & m[:, 0].le(S - 1) & m[:, 1].ge(0) & m[:, 1].le(S - 1)
        masks.append(norm.le(10) & inside)
        edge = torch.minimum(m.abs(), (m - (S - 1)).abs()).amin(dim=1)
        margins.append(torch.minimum((norm - 10).abs(), edge))
        src = ((rgb[:, 1 - d].double() + 1) * 127.5).permute(0, 3, 1, 2)
        warped.append(ssim_ref.sample_taps(src, ix, iy).permute(0, 2, 3, 1))
    return {"warped": torch.stack(warped), "mask": torch.stack(masks), "margin": torch.stack(margins)}


@functools.lru_cache(maxsize=None)
def panel_case(B, S, s):
    """(rgb, f0, f1, panels64 of them) of ssim_ref.case(B, S, S, s): computed once per process, shared, never written to."""
    rgb, f0, f1 = ssim_ref.case(B, S, S, s)
    return rgb, f0, f1, panels64(rgb, f0, f1)


@functools.lru_cache(maxsize=None)
def fractional_case():
    """A scale the reference's 256 / 64 never meets: 40 x 40 images under 16 x 16 flows, S / h = 2.5 and h / S = 0.4, which
    fp32 does not hold exactly.  (rgb, f0, f1, panels64 of them)."""
    rgb = ssim_ref.case(2, 40, 40, 4)[0]
    _, f0, f1 = ssim_ref.case(2, 48, 48, 3)
    return rgb, f0, f1, panels64(rgb, f0, f1)


def compare_panels(warped, mask, overlay, ref):
    """The figures every comparison of flow panels (fp32 stock ops, or the kernel's) against panels64 asserts on: share of
    pixels inside the exclusion band, mask mismatches outside it, share of true pixels, largest warped-value error, and of
    the overlay against the float64 chain outside the band: largest grey-level difference and share of differing elements."""
    keep = ref["margin"] >= BAND
    want = overlay_rule(ref["warped"], ref["mask"]).to(torch.int32)
    diff = (overlay.cpu().to(torch.int32) - want).abs()[keep]
    return {"band": 1.0 - float(keep.double().mean()),
            "mask_mismatch": int((mask.cpu().bool() != ref["mask"])[keep].sum()),
            "true": float(ref["mask"].double().mean()),
            "warped_err": float((warped.cpu().double() - ref["warped"]).abs().max()),
            "overlay_max": int(diff.max()), "overlay_share": float((diff != 0).double().mean())}


def entropy_cases(rows, S):
    """{name: at_wt (rows, S) fp32}: uniform, one-hot (zeros present), peaked, and uniform with one NaN row."""
    g = torch.Generator().manual_seed(1000 * rows + S)
    uniform = torch.full((rows, S), 1.0 / S)
    onehot = torch.zeros(rows, S)
    onehot[torch.arange(rows), torch.randint(0, S, (rows,), generator=g)] = 1.0
    peaked = torch.softmax(8.0 * torch.randn(rows, S, generator=g), dim=-1)
    nanrow = torch.softmax(torch.randn(rows, S, generator=g), dim=-1)
    nanrow[rows // 2, S // 2] = float("nan")
    return {"uniform": uniform, "onehot": onehot, "peaked": peaked, "nanrow": nanrow}


ENTROPY_SHAPES = ((1, 1), (5, 37), (3, 64), (7, 128), (4099, 200))


def entropy64(at_wt, nan_to_zero=False):
    """The mean row entropy in float64 with the argument of the logarithm GIVEN in fp32: x = fl32(w + 1e-5) is the reference's
    first operation, one IEEE addition that every fp32 form shares, and at w = 1 its rounding is 0.6 % of log(x) - a float64
    run on its own sum measures that rounding, not the code under test."""
    x = (at_wt + 1e-5).double()
    ent = -(at_wt.double() * torch.log(x)).sum(dim=-1)
    if nan_to_zero:
        ent = torch.where(torch.isnan(ent), torch.zeros_like(ent), ent)
    return ent.mean()


def entropy_bound(at_wt):
    """What |fp32 result - entropy64| may be, from the term count: a row of S terms t = w log(x) carries, relative to
    sum |t|, the logarithm (2 U: 1 ulp), the product (U) and up to S additions in any order (S U); the mean over the rows adds
    the fp32 additions of a workgroup's 32 rows (32 U); the float64 finish and the rounding of the result 2 U.  NaN rows are
    left out of the sum (they are either the whole result or count as 0)."""
    S = at_wt.shape[-1]
    t = (at_wt.double() * torch.log((at_wt + 1e-5).double())).abs().reshape(-1, S).sum(-1)
    t = torch.where(torch.isnan(t), torch.zeros_like(t), t)
    return float((S + 2 + 1 + 32 + 2) * U * t.mean())
