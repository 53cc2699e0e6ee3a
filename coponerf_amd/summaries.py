"""The reference's training / validation log (summary/summaries.py:img_summaries, wrapper.py:126-130), kept on the device.

img_summaries turns every validation batch into TensorBoard images and scalars through two F.interpolate and four
grid_sample calls, a Python loop with a `.cpu().numpy()` per image and direction, the depth map copied to the host for a
matplotlib colour map and a `.cpu()` per grid; every one of those host reads waits for the render.  Here

  attention_entropy  mean_rows(-sum w log(w + 1e-5)) of at_wt: csrc/summaries.hip, 2 launches      summaries.py:114-117, wrapper.py:126-130
  flow_panels        warped source, validity mask and mask overlay of both directions, 1 launch    summaries.py:163-207, 42-63, 74-100
  depth_colors       matplotlib's `jet` of depth / 10 as a table lookup, 1 launch                   summaries.py:129-133
  make_grid          torchvision.utils.make_grid at the defaults the reference uses, stock ops      summaries.py:124, 137, ...
  image_summaries    every image and scalar of img_summaries as device tensors under its tags       summaries.py:106-235
  SummaryLog         packs a Summary into ONE pinned buffer with one asynchronous copy and writes   test.py:270, wrapper.py:240
                     it `lag` calls later, when no render waits for it

  epipolar_lines     two_view_geometry and the epilines' end points in float64: csrc/epipolar.hip, 1 launch   inspect_epipolar_geometry.py:13-43, 54-55
  epipolar_panels    the nine dots on view 1 and their epipolar lines on view 0, under the estimated    inspect_epipolar_geometry.py:46-57, 75-120
                     and under the true pose, whole batch: 2 launches (the lines, the pixels)
  mask_contour       the 1-pixel contour of overlay_semantic_mask around the invalid region, 1 launch    summaries.py:65-71

The two OpenCV pieces are opt-in (`epipolar=True`, `contour=True` of image_summaries / SummaryLog): by default the tags
`epipolar_GT` / `epipolar_pred` are not written and `masked_warped_img*` carry no contour, as before.  Which pixels a disc, a
thick line and the contour cover is this package's own definition (include/coponerf_hip.h); `cv2` was not available, so
agreement with OpenCV's rasteriser on edge pixels has not been checked.  Where the reference's inspect() raises (a line with
b == 0, a non-finite pose, an end point beyond int32) its `except` drops both images for the whole batch; here that one line
is left out and everything else is drawn.  The epilines are not scaled to a^2 + b^2 = 1 (the drawing does not depend on it),
and a pixel no line covers keeps its value instead of passing through 0.4 v + 0.6 v.

Left out: drawpoint (inspect_epipolar_geometry.py:59-69), which nothing upstream calls.
"""
from __future__ import annotations

import math
from collections import deque
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from . import _hip

IMAGE_TAGS = ("predictions", "depth_images", "context_images", "query_images", "warped_img", "masked_warped_img",
              "warped_img_flip", "masked_warped_img_flip")
EPIPOLAR_TAGS = ("epipolar_GT", "epipolar_pred")            # written after IMAGE_TAGS, in this order (summaries.py:213-219)

# inspect_epipolar_geometry.py:83-84: the nine points are the {S/4, S/2, 3S/4}^2 grid (64 / 128 / 192 at S = 256), x outermost
EPIPOLAR_COLORS = ((63, 228, 92), (222, 155, 167), (56, 220, 130), (216, 43, 206), (47, 172, 72), (198, 181, 0), (137, 99, 246),
                   (22, 160, 10), (23, 240, 252))

# matplotlib's `jet` (matplotlib/_cm.py, public since 0.x): piecewise-linear through these (x, y) nodes per channel
_JET_NODES = (
    ((0.0, 0.0), (0.35, 0.0), (0.66, 1.0), (0.89, 1.0), (1.0, 0.5)),
    ((0.0, 0.0), (0.125, 0.0), (0.375, 1.0), (0.64, 1.0), (0.91, 0.0), (1.0, 0.0)),
    ((0.0, 0.5), (0.11, 1.0), (0.34, 1.0), (0.65, 0.0), (1.0, 0.0)),
)


def jet_table() -> np.ndarray:
    """(256, 3) float64: LinearSegmentedColormap('jet', N=256)'s lookup table, the interpolation at i / 255 of the nodes."""
    x = np.linspace(0.0, 1.0, 256)
    return np.stack([np.interp(x, [p[0] for p in nodes], [p[1] for p in nodes]) for nodes in _JET_NODES], axis=-1)


_JET_DEVICE: Dict[torch.device, torch.Tensor] = {}


def _jet_on(dev: torch.device) -> torch.Tensor:
    t = _JET_DEVICE.get(dev)
    if t is None:
        t = _JET_DEVICE[dev] = torch.from_numpy(jet_table().astype(np.float32)).pin_memory().to(dev, non_blocking=True)
    return t


def _device_tensor(name: str, what: str, t, dtype: torch.dtype, kind: str) -> None:
    if not torch.is_tensor(t):
        raise TypeError(f"{name}: {what} must be a tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name} runs on the HIP device only (coponerf_amd has no non-HIP compute path)")
    if t.dtype != dtype:
        raise ValueError(f"{name}: {kind} tensors only, {what} is {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: {what} must be contiguous")


def _device_f32(name: str, what: str, t) -> None:
    _device_tensor(name, what, t, torch.float32, "fp32")


def default_points(S: int) -> Tuple[Tuple[int, int], ...]:
    """The reference's nine points (x, y) for images of side S, in its order."""
    at = (S // 4, S // 2, 3 * S // 4)
    return tuple((x, y) for x in at for y in at)


_SETTINGS_DEVICE: Dict[tuple, torch.Tensor] = {}


def _settings_on(dev: torch.device, values, dtype: torch.dtype) -> torch.Tensor:
    """A small table of settings (points, colours) on the device: uploaded once per value from pinned memory, asynchronously."""
    key = (dev, dtype, tuple(tuple(v) for v in values))
    t = _SETTINGS_DEVICE.get(key)
    if t is None:
        t = _SETTINGS_DEVICE[key] = torch.tensor(key[2], dtype=dtype).pin_memory().to(dev, non_blocking=True)
    return t


# ---------------------------------------------------------------------------------------------------------- the kernels
def attention_entropy(at_wt: torch.Tensor, nan_to_zero: bool = False) -> torch.Tensor:
    """0-dim fp32 on the device: mean over the rows of -sum_s w log(w + 1e-5), at_wt (..., S) read once.  nan_to_zero=False
    is summaries.py:116-117 (a NaN row makes the result NaN); True is wrapper.py:128-130 (a NaN row counts as 0)."""
    _device_f32("attention_entropy", "at_wt", at_wt)
    if at_wt.dim() < 1 or at_wt.numel() == 0:
        raise ValueError(f"attention_entropy: need at least one row of at least one weight, got {tuple(at_wt.shape)}")
    S = int(at_wt.shape[-1])
    rows = at_wt.numel() // S
    nblk = _hip.lib().cpn_attention_entropy_blocks(rows)
    if nblk <= 0:
        raise ValueError(f"attention_entropy: {rows} rows are too many for one launch")
    partial = torch.empty(nblk, dtype=torch.float32, device=at_wt.device)
    out = torch.empty(1, dtype=torch.float32, device=at_wt.device)
    with torch.cuda.device(at_wt.device):
        _hip.call("cpn_attention_entropy", at_wt.data_ptr(), rows, S, 1 if nan_to_zero else 0, partial.data_ptr(), out.data_ptr(),
                  _hip.stream_handle())
    return out[0]


def flow_panels(context_rgb: torch.Tensor, flow: Sequence[torch.Tensor],
                contour: bool = False) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(warped (2, B, S, S, 3) fp32 in [0, 255], mask (2, B, S, S) uint8, overlay (2, B, S, S, 3) uint8) of
    summaries.py:163-207: entry d warps view 1 - d of context_rgb (B, 2, S, S, 3) by flow[d] (B, 2, h, h), upsampled
    bilinearly and scaled by S / h; the mask is the cycle check (norm <= 10) times get_gt_correspondence_mask; the overlay
    is overlay_semantic_mask(color=[255, 102, 51], alpha=0.5), with its contour (mask_contour) when contour=True.  Any
    square S >= h."""
    f0, f1 = flow[0], flow[1]
    for what, t in (("context_rgb", context_rgb), ("flow[0]", f0), ("flow[1]", f1)):
        _device_f32("flow_panels", what, t)
    if context_rgb.dim() != 5 or context_rgb.shape[1] != 2 or context_rgb.shape[4] != 3 or context_rgb.shape[2] != context_rgb.shape[3]:
        raise ValueError(f"flow_panels: context_rgb must be (B, 2, S, S, 3), got {tuple(context_rgb.shape)}")
    B, S = int(context_rgb.shape[0]), int(context_rgb.shape[2])
    if f0.dim() != 4 or f0.shape != f1.shape or f0.shape[0] != B or f0.shape[1] != 2 or f0.shape[2] != f0.shape[3]:
        raise ValueError(f"flow_panels: two (B, 2, h, h) flows for B = {B}, got {tuple(f0.shape)} and {tuple(f1.shape)}")
    h = int(f0.shape[2])
    if B < 1 or h < 1 or S < h:
        raise ValueError(f"flow_panels: need B >= 1 and S >= h >= 1, got B = {B}, S = {S}, h = {h}")
    if f0.device != context_rgb.device or f1.device != context_rgb.device:
        raise ValueError("flow_panels: images and flows are on different devices")
    dev = context_rgb.device
    warped = torch.empty(2, B, S, S, 3, dtype=torch.float32, device=dev)
    mask = torch.empty(2, B, S, S, dtype=torch.uint8, device=dev)
    overlay = torch.empty(2, B, S, S, 3, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _hip.call("cpn_flow_panels", context_rgb.data_ptr(), f0.data_ptr(), f1.data_ptr(), B, S, h, warped.data_ptr(),
                  mask.data_ptr(), overlay.data_ptr(), _hip.stream_handle())
    if contour:
        overlay = mask_contour(overlay, mask)
    return warped, mask, overlay


def mask_contour(overlay: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """A new overlay (..., S, S, 3) uint8 with the 1-pixel contour of summaries.py:65-71: exactly (255, 102, 51) on every
    invalid pixel (mask (..., S, S) uint8 == 0) with a valid or outside-the-image 4-neighbour - the border points that
    cv2.findContours follows and drawContours(thickness=1) repaints - and the overlay's value elsewhere.  One launch."""
    _device_tensor("mask_contour", "overlay", overlay, torch.uint8, "uint8")
    _device_tensor("mask_contour", "mask", mask, torch.uint8, "uint8")
    if (overlay.dim() < 3 or overlay.shape[-1] != 3 or overlay.shape[-2] != overlay.shape[-3] or mask.shape != overlay.shape[:-1]
            or overlay.numel() == 0):
        raise ValueError(f"mask_contour: overlay (..., S, S, 3) and mask (..., S, S), got {tuple(overlay.shape)} and {tuple(mask.shape)}")
    if mask.device != overlay.device:
        raise ValueError("mask_contour: overlay and mask are on different devices")
    S = int(overlay.shape[-2])
    out = torch.empty_like(overlay)
    with torch.cuda.device(overlay.device):
        _hip.call("cpn_mask_contour", overlay.data_ptr(), mask.data_ptr(), mask.numel() // (S * S), S, out.data_ptr(),
                  _hip.stream_handle())
    return out


def _check_geometry(name: str, intrinsics, rel_pose, gt_rel_pose) -> int:
    for what, t in (("intrinsics", intrinsics), ("rel_pose", rel_pose), ("gt_rel_pose", gt_rel_pose)):
        _device_f32(name, what, t)
    if intrinsics.dim() != 4 or tuple(intrinsics.shape[1:]) != (2, 4, 4) or intrinsics.shape[0] < 1:
        raise ValueError(f"{name}: intrinsics must be (B, 2, 4, 4), got {tuple(intrinsics.shape)}")
    B = int(intrinsics.shape[0])
    if tuple(rel_pose.shape) != (B, 4, 4) or tuple(gt_rel_pose.shape) != (B, 4, 4):
        raise ValueError(f"{name}: rel_pose and gt_rel_pose must be (B, 4, 4) for B = {B}, got {tuple(rel_pose.shape)} and "
                         f"{tuple(gt_rel_pose.shape)}")
    if rel_pose.device != intrinsics.device or gt_rel_pose.device != intrinsics.device:
        raise ValueError(f"{name}: intrinsics and poses are on different devices")
    return B


def _check_points(name: str, points, dev: torch.device) -> int:
    _device_tensor(name, "points", points, torch.int32, "int32")
    if points.dim() != 2 or points.shape[1] != 2 or points.shape[0] < 1:
        raise ValueError(f"{name}: points must be (P, 2) with P >= 1, got {tuple(points.shape)}")
    if points.device != dev:
        raise ValueError(f"{name}: points are on another device")
    return int(points.shape[0])


def epipolar_lines(intrinsics: torch.Tensor, rel_pose: torch.Tensor, gt_rel_pose: torch.Tensor, points: torch.Tensor,
                   width: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(F (2, B, 3, 3) float64, lines (2, B, P, 3) float64, ends (2, B, P, 4) int32, valid (2, B, P) uint8); entry 0 under
    rel_pose, entry 1 under gt_rel_pose.  two_view_geometry (inspect_epipolar_geometry.py:13-43) in float64 from the fp32
    inputs: F = inv(K_view0[:3,:3]).T [t]x R inv(K_view1[:3,:3]) of intrinsics (B, 2, 4, 4), each inverse rounded to fp32 as
    np.linalg.inv returns it for an fp32 matrix; line p = F (x, y, 1) of points
    (P, 2) int32 in view 1; ends = (0, int(-c / b), width, int(-(c + a width) / b)) as drawpointslines forms them; valid is 0
    where b == 0, a value is not finite or an end point does not fit an int32.  One launch."""
    B = _check_geometry("epipolar_lines", intrinsics, rel_pose, gt_rel_pose)
    P = _check_points("epipolar_lines", points, intrinsics.device)
    width = int(width)
    if width < 1:
        raise ValueError(f"epipolar_lines: width must be >= 1, got {width}")
    dev = intrinsics.device
    Fm = torch.empty(2, B, 3, 3, dtype=torch.float64, device=dev)
    lines = torch.empty(2, B, P, 3, dtype=torch.float64, device=dev)
    ends = torch.empty(2, B, P, 4, dtype=torch.int32, device=dev)
    valid = torch.empty(2, B, P, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _hip.call("cpn_epipolar_lines", intrinsics.data_ptr(), rel_pose.data_ptr(), gt_rel_pose.data_ptr(), points.data_ptr(), B, P,
                  width, Fm.data_ptr(), lines.data_ptr(), ends.data_ptr(), valid.data_ptr(), _hip.stream_handle())
    return Fm, lines, ends, valid


def epipolar_panels(context_rgb: torch.Tensor, intrinsics: torch.Tensor, rel_pose: torch.Tensor, gt_rel_pose: torch.Tensor,
                    points: Optional[torch.Tensor] = None, colors: Optional[torch.Tensor] = None, radius: int = 5,
                    thickness: int = 10) -> Tuple[torch.Tensor, torch.Tensor]:
    """(pred, gt), each (B, S, 2 S, 3) fp32 in [0, 255]: inspect() of inspect_epipolar_geometry.py:75-120 for context_rgb
    (B, 2, S, S, 3).  Left half: view 1 with a disc of `radius` at every point; right half: view 0 with the points' epipolar
    lines of `thickness`, blended 0.4 colour + 0.6 image; under rel_pose and under gt_rel_pose.  points (P, 2) int32 (x, y)
    and colors (P, 3) fp32 on the device; None takes the reference's nine points and colours.  2 launches, no host read."""
    name = "epipolar_panels"
    _device_f32(name, "context_rgb", context_rgb)
    if context_rgb.dim() != 5 or context_rgb.shape[1] != 2 or context_rgb.shape[4] != 3 or context_rgb.shape[2] != context_rgb.shape[3]:
        raise ValueError(f"{name}: context_rgb must be (B, 2, S, S, 3), got {tuple(context_rgb.shape)}")
    dev, S = context_rgb.device, int(context_rgb.shape[2])
    B = _check_geometry(name, intrinsics, rel_pose, gt_rel_pose)
    if B != context_rgb.shape[0] or S < 1:
        raise ValueError(f"{name}: {B} intrinsics for context_rgb of shape {tuple(context_rgb.shape)}")
    if intrinsics.device != dev:
        raise ValueError(f"{name}: images and intrinsics are on different devices")
    if points is None:
        points = _settings_on(dev, default_points(S), torch.int32)
    P = _check_points(name, points, dev)
    if colors is None:
        if P != len(EPIPOLAR_COLORS):
            raise ValueError(f"{name}: pass colors (P, 3) for {P} points")
        colors = _settings_on(dev, EPIPOLAR_COLORS, torch.float32)
    _device_f32(name, "colors", colors)
    if tuple(colors.shape) != (P, 3) or colors.device != dev:
        raise ValueError(f"{name}: colors must be ({P}, 3) on the images' device, got {tuple(colors.shape)}")
    radius, thickness = int(radius), int(thickness)
    if not (0 <= radius <= 255 and 1 <= thickness <= 255):
        raise ValueError(f"{name}: need 0 <= radius <= 255 and 1 <= thickness <= 255, got {radius} and {thickness}")
    _, _, ends, valid = epipolar_lines(intrinsics, rel_pose, gt_rel_pose, points, S)
    out = torch.empty(2, B, S, 2 * S, 3, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _hip.call("cpn_epipolar_panels", context_rgb.data_ptr(), points.data_ptr(), colors.data_ptr(), ends.data_ptr(),
                  valid.data_ptr(), B, S, P, radius, thickness, out.data_ptr(), _hip.stream_handle())
    return out[0], out[1]


def depth_colors(depth_ray: torch.Tensor) -> torch.Tensor:
    """depth_ray.shape + (3,) fp32: plt.get_cmap("jet")(depth / 10)[..., :3] as summaries.py:129-132 evaluates it on a
    float32 array (NaN -> 0 0 0, below 0 -> the first entry, 10 and above -> the last)."""
    _device_f32("depth_colors", "depth_ray", depth_ray)
    if depth_ray.numel() == 0:
        raise ValueError("depth_colors: empty depth_ray")
    out = torch.empty(*depth_ray.shape, 3, dtype=torch.float32, device=depth_ray.device)
    with torch.cuda.device(depth_ray.device):
        _hip.call("cpn_depth_jet", depth_ray.data_ptr(), depth_ray.numel(), _jet_on(depth_ray.device).data_ptr(), out.data_ptr(),
                  _hip.stream_handle())
    return out


# ------------------------------------------------------------------------------------------------------------ the grids
def make_grid(images: torch.Tensor, normalize: bool = True, scale_each: bool = False) -> torch.Tensor:
    """torchvision.utils.make_grid(images, nrow=8, padding=2, pad_value=0, normalize=..., scale_each=...) of (N, C, H, W)
    images, C in {1, 3}, on the images' device (CPU tensors too).  No value is read on the host: the minimum and maximum
    stay tensors, the divisor max - min + 1e-5 is formed in float64 as the Python floats of torchvision are."""
    if images.dim() != 4 or images.shape[1] not in (1, 3) or images.shape[0] < 1:
        raise ValueError(f"make_grid: (N, 1 or 3, H, W) images, got {tuple(images.shape)}")
    t = images
    if t.shape[1] == 1:
        t = t.expand(-1, 3, -1, -1)
    if normalize:                                           # torchvision's clamp to [min, max] changes nothing: they are t's own
        dims = (1, 2, 3) if scale_each else (0, 1, 2, 3)
        lo, hi = t.amin(dim=dims, keepdim=True), t.amax(dim=dims, keepdim=True)
        t = (t - lo) / (hi.double() - lo.double() + 1e-5).to(t.dtype)
    N, C, H, W = t.shape
    if N == 1:
        return t[0]
    xmaps = min(8, N)
    ymaps = -(-N // xmaps)
    grid = t.new_zeros(C, ymaps * (H + 2) + 2, xmaps * (W + 2) + 2)
    for y in range(ymaps):                                  # one strided copy per row of the grid
        row = t[y * xmaps:(y + 1) * xmaps]
        cells = grid[:, y * (H + 2) + 2:y * (H + 2) + 2 + H, 2:].unflatten(2, (xmaps, W + 2))
        cells[:, :, :row.shape[0], :W] = row.permute(1, 2, 0, 3)
    return grid


class Summary:
    """What img_summaries writes for one batch: `images` tag -> (3, h, w) fp32 grid, `scalars` tag -> 0-dim fp32, all on
    the device, in the reference's order of writing."""

    def __init__(self, images: Dict[str, torch.Tensor], scalars: Dict[str, torch.Tensor]):
        self.images = images
        self.scalars = scalars


def _image_shape(rgb: torch.Tensor, image_shape: Optional[Sequence[int]]) -> Tuple[int, int]:
    if image_shape is not None:
        return int(image_shape[0]), int(image_shape[1])
    R = int(rgb.shape[-2])
    side = math.isqrt(R)
    if side * side != R:
        raise ValueError(f"image_summaries: pass image_shape=(H, W) for rgb of shape {tuple(rgb.shape)}")
    return side, side


@torch.no_grad()
def image_summaries(model_input: Dict, model_output: Dict, image_shape: Optional[Sequence[int]] = None, epipolar: bool = False,
                    contour: bool = False) -> Summary:
    """summaries.py:106-235 for one batch, without its writer: model_output is the joined dict of `forward(val=True)` /
    `render_images` ('rgb', 'depth_ray', 'flow', 'rel_pose', 'gt_rel_pose', optionally 'at_wt'), model_input the loader's dict
    on the device.  image_shape=(H, W) of the query image; None takes it as square.  epipolar=True adds EPIPOLAR_TAGS after
    IMAGE_TAGS (it reads model_input['context']['intrinsics']); contour=True draws the contour on the two masked images.
    Enqueues device work only."""
    rgb = model_output["rgb"]
    H, W = _image_shape(rgb, image_shape)
    images: Dict[str, torch.Tensor] = {}
    scalars: Dict[str, torch.Tensor] = {}

    predictions = rgb.reshape(-1, H, W, 3).permute(0, 3, 1, 2).clamp(-1, 1)
    if "at_wt" in model_output:
        scalars["ent"] = attention_entropy(model_output["at_wt"].contiguous())
    images["predictions"] = make_grid(predictions)
    depth = depth_colors(model_output["depth_ray"].contiguous()).reshape(-1, H, W, 3).permute(0, 3, 1, 2)
    images["depth_images"] = make_grid(depth, scale_each=True)
    ctx = model_input["context"]["rgb"]
    images["context_images"] = make_grid(ctx.flatten(0, 1).permute(0, 3, 1, 2))
    query = model_input["query"]["rgb"].reshape(-1, H, W, 3).permute(0, 3, 1, 2)
    images["query_images"] = make_grid(query)

    flow = model_output["flow"]
    warped, _, overlay = flow_panels(ctx.contiguous(), (flow[0].contiguous(), flow[1].contiguous()), contour=contour)
    view255 = (ctx + 1) * 127.5
    for d, suffix in ((0, ""), (1, "_flip")):
        panel = torch.cat((view255[:, 1 - d], warped[d], view255[:, d]), dim=-2)          # [source | warped | target]
        images["warped_img" + suffix] = make_grid(panel.permute(0, 3, 1, 2))
        images["masked_warped_img" + suffix] = make_grid(overlay[d].float().permute(0, 3, 1, 2))
    rel, gt_rel = model_output["rel_pose"], model_output["gt_rel_pose"]
    if epipolar:
        pred, gt = epipolar_panels(ctx.contiguous(), model_input["context"]["intrinsics"].contiguous(), rel.contiguous(),
                                   gt_rel.contiguous())
        images["epipolar_GT"] = make_grid(gt.permute(0, 3, 1, 2))
        images["epipolar_pred"] = make_grid(pred.permute(0, 3, 1, 2))

    S, h = int(ctx.shape[2]), int(flow[0].shape[2])
    scalars["flow_mean"] = (F.interpolate(flow[0][:1, :1], S, mode="bilinear") * (S / h)).mean()     # image 0, x component
    scalars["out_min"], scalars["out_max"] = predictions.min(), predictions.max()
    m = torch.bmm(rel[:, :3, :3], gt_rel[:, :3, :3].transpose(1, 2))
    theta = torch.acos(((m[:, 0, 0] + m[:, 1, 1] + m[:, 2, 2] - 1) / 2).clamp(-1.0, 1.0))
    degrees = theta / np.pi * 180
    scalars["rot_distance"] = theta.mean()
    scalars["rot_distance_degrees_mean"] = degrees.mean()
    scalars["rot_distance_degrees_std"] = degrees.std()
    scalars["rot_distance_degrees_max"] = degrees.max()
    scalars["tran_L1"] = F.mse_loss(rel[:, :3, 3], gt_rel[:, :3, 3])                                  # an MSE upstream too
    scalars["trgt_min"], scalars["trgt_max"] = query.min(), query.max()
    return Summary(images, scalars)


# -------------------------------------------------------------------------------------------------------------- the log
class SummaryLog:
    """Writes Summaries through a TensorBoard-style writer (`add_image(tag, chw_numpy, step)`, `add_scalar(tag, value, step)`)
    without making a render wait:

        log = SummaryLog(writer, prefix="val_", lag=1)
        for step, (inp, out) in enumerate(render_images(model, inputs)):
            log.add(inp, out, step)              # enqueues; writes the entry added `lag` calls earlier
        log.flush()

    `add` packs every image and scalar into ONE flat pinned buffer with one asynchronous copy and records an event; the
    entry is written once `lag` newer ones exist (its copy finished long ago) or at `flush`.  `host_reads` counts one per
    written entry.  `epipolar` and `contour` are image_summaries' switches."""

    def __init__(self, writer, prefix: str = "", lag: int = 1, epipolar: bool = False, contour: bool = False):
        if lag < 0:
            raise ValueError(f"SummaryLog: lag must be >= 0, got {lag}")
        self.writer = writer
        self.prefix = prefix
        self.lag = int(lag)
        self.epipolar, self.contour = bool(epipolar), bool(contour)
        self.host_reads = 0
        self._pending: deque = deque()
        self._free: Dict[int, List[torch.Tensor]] = {}

    def __len__(self) -> int:
        return len(self._pending)

    def _pinned(self, n: int) -> torch.Tensor:
        pool = self._free.get(n)
        return pool.pop() if pool else torch.empty(n, dtype=torch.float32, pin_memory=True)

    @torch.no_grad()
    def add(self, model_input: Dict, model_output: Dict, step: int, image_shape: Optional[Sequence[int]] = None) -> None:
        summary = image_summaries(model_input, model_output, image_shape, epipolar=self.epipolar, contour=self.contour)
        while len(self._pending) > max(self.lag - 1, 0):
            self._write(self._pending.popleft())
        layout = [(tag, True, tuple(t.shape)) for tag, t in summary.images.items()]
        layout += [(tag, False, ()) for tag in summary.scalars]
        flat = torch.cat([t.reshape(-1) for t in list(summary.images.values()) + list(summary.scalars.values())])
        host = self._pinned(flat.numel())
        host.copy_(flat, non_blocking=True)
        event = torch.cuda.Event()
        event.record()
        self._pending.append((step, layout, host, event))
        if self.lag == 0:
            self._write(self._pending.popleft())

    def _write(self, entry) -> None:
        step, layout, host, event = entry
        event.synchronize()
        self.host_reads += 1
        values = host.numpy()
        at = 0
        for tag, is_image, shape in layout:
            if is_image:
                n = int(np.prod(shape))
                self.writer.add_image(self.prefix + tag, values[at:at + n].reshape(shape).copy(), step)
            else:
                n = 1
                self.writer.add_scalar(self.prefix + tag, float(values[at]), step)
            at += n
        self._free.setdefault(host.numel(), []).append(host)

    def flush(self) -> None:
        while self._pending:
            self._write(self._pending.popleft())
