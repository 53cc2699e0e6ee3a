"""A PointCloud drawn into any camera through a z-buffer: the reconstruction made visible on a headless machine, and a check of
depth and estimated pose against the second photo that needs no ground truth.

  splat_points      the cloud into K cameras: a (K, B, H, W) z-buffer of (depth bits, point index) keys: cpn_splat_points
  resolve           a z-buffer -> frames, depth and index: cpn_splat_resolve
  draw              the two together: the (K, B, H, W, 3) uint8 frames render_path returns, far below the cost of a network render
  score             coverage and PSNR over the covered pixels of frames against a target: cpn_splat_score
  orbit_poses       K cameras on an arc about a pivot on view 0's optical axis (a turntable)
  cross_view_check  the cloud of ONE view drawn into the other view's estimated camera and scored against that photo, both ways

The footprint rule (a square of 2 radius + 1 pixels, whatever the depth), the fill rule (an empty pixel takes the nearest
point of the splatted neighbourhood, once), the tie rule (equal depths fall to the lower index) and cross_view_check are this
package's definitions (include/coponerf_hip.h), not the reference's, which has no point renderer.  None of it has been tried
on a trained checkpoint, because none is available offline.  Left out: perspective-sized points, blending and antialiasing,
triangles (coponerf_amd.mesh makes a mesh and coponerf_amd.raster draws it; Mesh.cloud() hands its vertices to draw), video
encoding.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _hip
from ._args import background_word, device_tensors, frame_outputs, one_device, view_cameras, zbuffer_dims
from .novel_views import pack_frames, render_path


def _cloud(who: str, cloud) -> Tuple[int, int]:
    xyz, rgb, count = cloud.xyz, cloud.rgb, cloud.count
    device_tensors(who, (("cloud.xyz", xyz, torch.float32, None), ("cloud.rgb", rgb, torch.uint8, None),
                         ("cloud.count", count, torch.int32, None)), owner="the cloud's device")
    if xyz.dim() != 3 or xyz.shape[2] != 3 or rgb.shape != xyz.shape or tuple(count.shape) != (int(xyz.shape[0]),):
        raise ValueError(f"{who}: a PointCloud of xyz (B, cap, 3), rgb (B, cap, 3) and count (B), got {tuple(xyz.shape)}, "
                         f"{tuple(rgb.shape)} and {tuple(count.shape)}")
    return int(xyz.shape[0]), int(xyz.shape[1])


@torch.no_grad()
def splat_points(cloud, poses: torch.Tensor, intrinsics: torch.Tensor, H: int, W: int, radius: int = 1,
                 near: float = 1e-3) -> torch.Tensor:
    """cpn_splat_points: the z-buffer (K, B, H, W) of the cloud in the cameras `poses` (K, B, 4, 4) fp32, camera to reference
    (camera_path's, orbit_poses'), with `intrinsics` (B, 4, 4) or (B, 1, 4, 4) fp32 of the H x W output image.  An int64 tensor
    holding uint64 keys: (bits of the fp32 depth) << 32 | point index, -1 (all ones) where no point fell."""
    H, W, radius = int(H), int(W), int(radius)
    B, cap = _cloud("splat_points", cloud)
    K, Kb = view_cameras("splat_points", poses, intrinsics, B, cap, H, W, cloud.xyz.device, "the cloud's device")
    if not 0 <= radius <= 8 or not float(near) > 0.0:
        raise ValueError(f"splat_points: need 0 <= radius <= 8 and near > 0, got {radius} and {near}")
    zbuf = torch.empty(K, B, H, W, dtype=torch.int64, device=cloud.xyz.device)
    with torch.cuda.device(zbuf.device):
        _hip.call("cpn_splat_points", cloud.xyz.data_ptr(), cloud.count.data_ptr(), poses.data_ptr(), Kb.data_ptr(), K, B, cap, H, W,
                  radius, float(near), zbuf.data_ptr(), _hip.stream_handle())
    return zbuf


@torch.no_grad()
def resolve(zbuf: torch.Tensor, rgb: torch.Tensor, fill: int = 0, background: Sequence[int] = (0, 0, 0),
            return_depth: bool = False, return_index: bool = False) -> Dict[str, torch.Tensor]:
    """cpn_splat_resolve: splat_points' z-buffer (K, B, H, W) and the cloud's rgb (B, cap, 3) uint8 -> `frames` (K, B, H, W, 3)
    uint8, on request `depth` (K, B, H, W) fp32 (NaN where empty) and `index` (K, B, H, W) int32 (-1 where empty).  fill > 0:
    an empty pixel takes the nearest point of the (2 fill + 1)^2 splatted pixels around it; background: the empty pixels' bytes."""
    one_device("resolve", zbuf, rgb)
    if rgb.dtype != torch.uint8 or rgb.dim() != 3 or rgb.shape[2] != 3:
        raise ValueError(f"resolve: rgb must be (B, cap, 3) uint8, got {tuple(rgb.shape)} {rgb.dtype}")
    K, B, H, W = zbuffer_dims("resolve", zbuf, int(rgb.shape[0]))
    cap, fill, word = int(rgb.shape[1]), int(fill), background_word("resolve", background)
    if not 0 <= fill <= 4:
        raise ValueError(f"resolve: need 0 <= fill <= 4, got {fill}")
    if not 1 <= K <= 255 or min(B, H, W, cap) < 1 or K * B * H * W >= 2 ** 31:
        raise ValueError(f"resolve: need 1 <= K <= 255, B, H, W, cap >= 1 and K B H W < 2^31, got {tuple(zbuf.shape)}, cap = {cap}")
    out, (frames, depth, index, _) = frame_outputs(K, B, H, W, zbuf.device, return_depth, return_index)
    with torch.cuda.device(zbuf.device):
        _hip.call("cpn_splat_resolve", zbuf.data_ptr(), rgb.data_ptr(), K, B, cap, H, W, fill, word, frames, depth, index,
                  _hip.stream_handle())
    return out


@torch.no_grad()
def draw(cloud, poses: torch.Tensor, intrinsics: torch.Tensor, H: int, W: int, radius: int = 1, fill: int = 0,
         near: float = 1e-3, background: Sequence[int] = (0, 0, 0), return_depth: bool = False,
         return_index: bool = False) -> Dict[str, torch.Tensor]:
    """The cloud as the K cameras `poses` see it: splat_points, then resolve.  Every point that lies at least `near` in front
    of a camera covers the (2 radius + 1)^2 pixels around the pixel it falls on; the nearest point wins a pixel, the lower
    index among equal depths.  Returns a dict of device tensors: `frames` (K, B, H, W, 3) uint8 as render_path's, with
    return_depth `depth` (K, B, H, W) fp32 (the z-depth in the camera, NaN where nothing fell), with return_index `index`
    (K, B, H, W) int32 (the row of the cloud, -1 where nothing fell).  Two launches and a memset; nothing is read on the host."""
    zbuf = splat_points(cloud, poses, intrinsics, H, W, radius=radius, near=near)
    return resolve(zbuf, cloud.rgb, fill=fill, background=background, return_depth=return_depth, return_index=return_index)


@torch.no_grad()
def score_counts(frames: torch.Tensor, index: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """cpn_splat_score: stats (K, B, 2) int64 = (the number n of pixels with index >= 0, the sum over them and their three
    channels of (frames - target)^2) of frames and target (K, B, H, W, 3) uint8 and index (K, B, H, W) int32."""
    one_device("score", frames, index, target)
    if frames.dtype != torch.uint8 or frames.dim() != 5 or frames.shape[4] != 3 or target.dtype != torch.uint8 or \
            target.shape != frames.shape or index.dtype != torch.int32 or index.shape != frames.shape[:4]:
        raise ValueError(f"score: frames and target (K, B, H, W, 3) uint8 and index (K, B, H, W) int32, got {tuple(frames.shape)} "
                         f"{frames.dtype}, {tuple(target.shape)} {target.dtype} and {tuple(index.shape)} {index.dtype}")
    K, B, H, W = (int(v) for v in index.shape)
    n_scratch = _hip.lib().cpn_splat_score_scratch(K, B, H, W)
    if n_scratch <= 0:
        raise ValueError(f"score: need 1 <= K <= 255, B, H, W >= 1 and K B H W < 2^31, got {tuple(index.shape)}")
    scratch = torch.empty(n_scratch, dtype=torch.int64, device=frames.device)
    stats = torch.empty(K, B, 2, dtype=torch.int64, device=frames.device)
    with torch.cuda.device(frames.device):
        _hip.call("cpn_splat_score", frames.data_ptr(), index.data_ptr(), target.data_ptr(), K, B, H, W, scratch.data_ptr(),
                  stats.data_ptr(), _hip.stream_handle())
    return stats


@torch.no_grad()
def score(frames: torch.Tensor, index: torch.Tensor, target: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(coverage (K, B), psnr (K, B)) float64 on the device of draw's frames and index against target (K, B, H, W, 3) uint8:
    coverage = n / (H W), the share of pixels a point fell on; psnr = 10 log10(255^2 . 3 n / sse) over those pixels, inf where
    they all agree and NaN where there are none.  Nothing is read on the host."""
    return coverage_psnr(score_counts(frames, index, target), int(index.shape[2]), int(index.shape[3]))


def coverage_psnr(stats: torch.Tensor, H: int, W: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """score's two float64 figures of cpn_splat_score's stats (..., 2) int64, on the tensor's own device."""
    n, sse = stats[..., 0].to(torch.float64), stats[..., 1].to(torch.float64)        # exact: both stay far below 2^53
    # a tensor as the divisor: by a Python number torch multiplies with the rounded reciprocal on the device
    return n / torch.full_like(n, float(H * W)), 10.0 * torch.log10(((255.0 ** 2 * 3.0) * n) / sse)


def orbit_matrices(K: int, pivot_z: float, yaw_deg: float, pitch_deg: float = 0.0) -> np.ndarray:
    """orbit_poses' (K, 4, 4) float64 matrices on the host.  Camera k is view 0's camera turned about the pivot
    p = (0, 0, pivot_z) of view 0's frame: R_k = R_y(yaw_k) R_x(pitch) (x right, y down, z forward), position p - R_k p, so
    that p stays on the optical axis at the distance pivot_z.  yaw_k is spaced evenly over [-yaw_deg, +yaw_deg]
    (np.linspace; K = 1: the middle, 0)."""
    K = int(K)
    if K < 1:
        raise ValueError(f"orbit_poses: need at least one camera, got K = {K}")
    yaw = np.deg2rad(np.linspace(-float(yaw_deg), float(yaw_deg), K) if K > 1 else np.zeros(1))
    cp, sp = np.cos(np.deg2rad(float(pitch_deg))), np.sin(np.deg2rad(float(pitch_deg)))
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, cp, -sp], [0.0, sp, cp]])
    pivot = np.array([0.0, 0.0, float(pivot_z)])
    out = np.zeros((K, 4, 4), dtype=np.float64)
    for k in range(K):
        c, s = np.cos(yaw[k]), np.sin(yaw[k])
        R = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]]) @ Rx
        out[k, :3, :3], out[k, :3, 3], out[k, 3, 3] = R, pivot - R @ pivot, 1.0
    return out


def orbit_poses(B: int, K: int, pivot_z: float, yaw_deg: float, pitch_deg: float = 0.0,
                device: Optional[torch.device] = None) -> torch.Tensor:
    """(K, B, 4, 4) fp32 on the device (the current one unless `device` names another): K cameras that look at the pivot
    (0, 0, pivot_z) of view 0's frame, turned about it by yaw angles spaced evenly over [-yaw_deg, +yaw_deg] and by pitch_deg
    (orbit_matrices: float64 numpy on the host, rounded to fp32 once and uploaded once; the same cameras for every pair).
    The pivot is the caller's number - the depth of what the photos show; nothing reads a cloud's centroid from the device."""
    B = int(B)
    if B < 1:
        raise ValueError(f"orbit_poses: need at least one pair, got B = {B}")
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        raise RuntimeError("orbit_poses uploads to the HIP device (coponerf_amd has no non-HIP compute path)")
    M = torch.from_numpy(orbit_matrices(K, pivot_z, yaw_deg, pitch_deg).astype(np.float32))
    host = torch.empty(int(K), B, 4, 4, dtype=torch.float32, pin_memory=True).copy_(M.unsqueeze(1).expand(int(K), B, 4, 4))
    return host.to(dev, non_blocking=True)


@torch.no_grad()
def cross_view_check(model, model_input: Dict, radius: int = 1, fill: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
    """Do depth and estimated pose agree with the other photo?  (coverage (2, B), psnr (2, B)) float64 on the device, needing
    nothing but the pair.

    render_path renders the two photos' own cameras (t = (0, 1)) once, with depth.  Direction 0: the cloud of view 0 ALONE
    (point_cloud.from_views on that view's slice, min_votes=0: every valid pixel, colours as the network rendered them) is
    drawn into view 1's estimated camera - camera_path(rel_pose, (1,)), which is render_path's `poses[1]` - with view 1's
    intrinsics, and scored against photo 1 (`context.rgb[:, 1]` as bytes, pack_frames).  Direction 1: the cloud of view 1 alone
    into view 0's camera, against photo 0.  No view scores its own pixels.  A high coverage with a low PSNR says that the
    geometry lands in the other photo but on the wrong content; a low coverage that the views share little or the depth
    is mostly invalid.  This package's definition; not tried on a trained checkpoint."""
    from .point_cloud import from_views
    ctx = model_input["context"]
    S = int(ctx["rgb"].shape[2])
    res = render_path(model, model_input, (0.0, 1.0), return_rgb=True, return_depth=True)
    scores = []
    for src in (0, 1):
        dst = 1 - src
        views = {k: res[k][src:src + 1].contiguous() for k in ("depth", "valid", "rgb", "poses")}
        cloud = from_views(views, model_input["query"]["intrinsics"], S, min_votes=0)
        out = draw(cloud, res["poses"][dst:dst + 1].contiguous(), ctx["intrinsics"][:, dst].contiguous(), S, S, radius=radius,
                   fill=fill, return_index=True)
        scores.append(score_photo(out, ctx["rgb"][:, dst]))
    return torch.stack([c for c, _ in scores]), torch.stack([p for _, p in scores])


def score_photo(out: Dict[str, torch.Tensor], photo: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(coverage (B), psnr (B)) of a draw into ONE camera (`frames` and `index` with K = 1: splat.draw's, raster.draw's) against
    the photo (B, H, W, 3) fp32 in [-1, 1] taken there, as bytes (pack_frames): what cross_view_check and raster.photo_check end in."""
    _, B, H, W = out["index"].shape
    target = pack_frames(photo.contiguous(), torch.empty(B, H, W, 3, dtype=torch.uint8, device=photo.device))
    coverage, psnr = score(out["frames"], out["index"], target.unsqueeze(0))
    return coverage[0], psnr[0]
