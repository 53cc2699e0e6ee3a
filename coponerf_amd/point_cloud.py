"""Two photos in, a fused coloured point cloud out: the model's geometry, kept on the device until the user asks for it.

`forward(val=True)` returns `depth_ray`: the z-depth, in the query camera, of the 3-D point of the ray's strongest sample,
clamped to [0, 10] (models/CoPoNeRF.py:509-540).  With the estimated pose that makes the model a two-view reconstruction
method; the reference has no script for it.  Here

  unproject     depth of K views -> points in view 0's frame: cpn_depth_points
  vote          forward-backward consistency of every pixel's depth with the other views, and the depth averaged over the
                views that agree: cpn_depth_votes
  reconstruct   novel_views.render_path for the K views, vote, unproject, select, cpn_compact_points -> a PointCloud
  PointCloud    xyz / rgb / count on the device; points(b) is the one host read, ply_bytes / save write a binary PLY

The validity rule (a depth counts iff it is finite and 0 < d < 10: both clamp ends are saturated values) and the vote rule
(include/coponerf_hip.h) are this package's definitions, not the reference's.  depth_ray is the depth of ONE of 2 x 64
samples, so a depth map is a staircase; the default thresholds (1 pixel, 1 %: the usual multi-view-stereo fusion values)
have not been tried on a trained checkpoint, because none is available offline.  Writing the PLY is the only file I/O.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _hip
from ._args import device_tensors, one_device, pair_intrinsics
from .novel_views import render_path


def _views(who: str, depth: torch.Tensor, poses: torch.Tensor, intrinsics: torch.Tensor, S: int,
           window: Optional[Sequence[int]]) -> Tuple[int, int, int, int, int, int, torch.Tensor]:
    """The checks unproject and vote share -> (K, B, y0, x0, h, w, the (B, 4, 4) intrinsics)."""
    device_tensors(who, (("depth", depth, torch.float32, None), ("poses", poses, torch.float32, None),
                         ("intrinsics", intrinsics, torch.float32, None)), owner="depth's device")
    if depth.dim() != 3 or poses.dim() != 4 or poses.shape[:2] != depth.shape[:2] or poses.shape[2:] != (4, 4):
        raise ValueError(f"{who}: depth (K, B, h * w) and poses (K, B, 4, 4), got {tuple(depth.shape)} and {tuple(poses.shape)}")
    K, B = int(depth.shape[0]), int(depth.shape[1])
    Kb = pair_intrinsics(who, intrinsics, B)
    S = int(S)
    y0, x0, h, w = (0, 0, S, S) if window is None else (int(v) for v in window)
    if not (0 <= y0 and 0 <= x0 and h >= 1 and w >= 1 and y0 + h <= S and x0 + w <= S):
        raise ValueError(f"{who}: window {(y0, x0, h, w)} does not lie in the {S} x {S} grid")
    if int(depth.shape[2]) != h * w:
        raise ValueError(f"{who}: depth of shape {tuple(depth.shape)} does not fill a window of {h} x {w}")
    if not 1 <= K <= 255 or B < 1 or K * B * h * w >= 2 ** 31:
        raise ValueError(f"{who}: need 1 <= K <= 255 views, B >= 1 and K B h w < 2^31, got K = {K}, B = {B}, h w = {h * w}")
    return K, B, y0, x0, h, w, Kb


@torch.no_grad()
def unproject(depth: torch.Tensor, poses: torch.Tensor, intrinsics: torch.Tensor, S: int,
              window: Optional[Sequence[int]] = None) -> torch.Tensor:
    """cpn_depth_points: depth (K, B, h * w) fp32 of the window (y0, x0, h, w) of an S x S grid (None: the whole grid), poses
    (K, B, 4, 4) fp32 camera to reference (camera_path's), intrinsics (B, 4, 4) or (B, 1, 4, 4) fp32 (`query.intrinsics`) ->
    xyz (K, B, h * w, 3) fp32 = pose . (d . ((u - cx) / fx, (v - cy) / fy, 1)), float64 inside; NaN where the depth is not
    valid (finite and 0 < d < 10)."""
    K, B, y0, x0, h, w, Kb = _views("unproject", depth, poses, intrinsics, S, window)
    xyz = torch.empty(K, B, h * w, 3, dtype=torch.float32, device=depth.device)
    with torch.cuda.device(depth.device):
        _hip.call("cpn_depth_points", depth.data_ptr(), poses.data_ptr(), Kb.data_ptr(), K, B, int(S), y0, x0, h, w, xyz.data_ptr(),
                  _hip.stream_handle())
    return xyz


@torch.no_grad()
def vote(depth: torch.Tensor, poses: torch.Tensor, intrinsics: torch.Tensor, S: int, px_tol: float, rel_tol: float,
         window: Optional[Sequence[int]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """cpn_depth_votes: (votes (K, B, h * w) uint8, depth_fused (K, B, h * w) fp32) of depth, poses and intrinsics as in
    unproject.  votes counts the other views whose own depth, read bilinearly where the pixel's point falls in them, brings
    the point back within px_tol pixels and rel_tol . d of where it started; depth_fused averages the pixel's depth with
    the depths those views bring back (NaN where the pixel's depth is not valid)."""
    K, B, y0, x0, h, w, Kb = _views("vote", depth, poses, intrinsics, S, window)
    if not (float(px_tol) >= 0.0 and float(rel_tol) >= 0.0):
        raise ValueError(f"vote: px_tol and rel_tol must be >= 0, got {px_tol} and {rel_tol}")
    votes = torch.empty(K, B, h * w, dtype=torch.uint8, device=depth.device)
    fused = torch.empty(K, B, h * w, dtype=torch.float32, device=depth.device)
    with torch.cuda.device(depth.device):
        _hip.call("cpn_depth_votes", depth.data_ptr(), poses.data_ptr(), Kb.data_ptr(), K, B, int(S), y0, x0, h, w, float(px_tol),
                  float(rel_tol), votes.data_ptr(), fused.data_ptr(), _hip.stream_handle())
    return votes, fused


@torch.no_grad()
def compact(keep: torch.Tensor, xyz: torch.Tensor, rgb: torch.Tensor, h: int, w: int) -> "PointCloud":
    """cpn_compact_points: keep (K, B, h * w) uint8 (non-zero = selected), xyz and rgb (K, B, h * w, 3) fp32 -> the PointCloud of
    the selected points of every pair in (view, row, column) order; its rows beyond the count are not written."""
    one_device("compact", keep, xyz, rgb)
    if keep.dtype != torch.uint8 or keep.dim() != 3 or int(keep.shape[2]) != h * w:
        raise ValueError(f"compact: keep must be (K, B, {h} * {w}) uint8, got {tuple(keep.shape)} {keep.dtype}")
    K, B = int(keep.shape[0]), int(keep.shape[1])
    for what, x in (("xyz", xyz), ("rgb", rgb)):
        if x.dtype != torch.float32 or tuple(x.shape) != (K, B, h * w, 3):
            raise ValueError(f"compact: {what} must be {(K, B, h * w, 3)} fp32, got {tuple(x.shape)} {x.dtype}")
    n_scratch = _hip.lib().cpn_compact_points_scratch(K, B, h, w)
    if n_scratch <= 0:
        raise ValueError(f"compact: need 1 <= K <= 255 views, 1 <= B <= 65535 and K B h w < 2^31, got K = {K}, B = {B}, h w = {h * w}")
    dev, cap = keep.device, K * h * w
    o_xyz = torch.empty(B, cap, 3, dtype=torch.float32, device=dev)
    o_rgb = torch.empty(B, cap, 3, dtype=torch.uint8, device=dev)
    count = torch.empty(B, dtype=torch.int32, device=dev)
    scratch = torch.empty(n_scratch, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _hip.call("cpn_compact_points", keep.data_ptr(), xyz.data_ptr(), rgb.data_ptr(), K, B, h, w, scratch.data_ptr(),
                  o_xyz.data_ptr(), o_rgb.data_ptr(), count.data_ptr(), _hip.stream_handle())
    return PointCloud(o_xyz, o_rgb, count)


class PointCloud:
    """The selected points of B pairs on the device: xyz (B, cap, 3) fp32 in view 0's frame, rgb (B, cap, 3) uint8 and count
    (B) int32; pair b's points are the rows [0, count[b]) in (view, row, column) order, the rows beyond are not written."""

    def __init__(self, xyz: torch.Tensor, rgb: torch.Tensor, count: torch.Tensor):
        self.xyz, self.rgb, self.count = xyz, rgb, count

    @torch.no_grad()
    def points(self, b: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        """Pair b's points on the host: ((n, 3) float32, (n, 3) uint8).  ONE read: the count, the positions and the colours
        of the pair travel in one buffer, the rows beyond the count are dropped on the host."""
        cap = int(self.xyz.shape[1])
        packed = torch.cat((self.count[b:b + 1].view(torch.uint8), self.xyz[b].view(torch.uint8).reshape(-1),
                            self.rgb[b].reshape(-1))).cpu().numpy()
        n = int(packed[:4].view(np.int32)[0])
        xyz = packed[4:4 + 12 * cap].view(np.float32).reshape(cap, 3)[:n].copy()
        rgb = packed[4 + 12 * cap:].reshape(cap, 3)[:n].copy()
        return xyz, rgb

    def ply_bytes(self, b: int = 0) -> bytes:
        """Pair b as a binary little-endian PLY: vertices of `float x y z`, `uchar red green blue`."""
        return ply_bytes(*self.points(b))

    def save(self, path, b: int = 0) -> None:
        with open(path, "wb") as f:
            f.write(self.ply_bytes(b))

    def frames(self, poses: torch.Tensor, intrinsics: torch.Tensor, H: int, W: int, **kwargs) -> Dict[str, torch.Tensor]:
        """The cloud as the cameras `poses` (K, B, 4, 4) see it, on the device: coponerf_amd.splat.draw(self, ...)."""
        from .splat import draw
        return draw(self, poses, intrinsics, H, W, **kwargs)


def ply_bytes(xyz: np.ndarray, rgb: np.ndarray) -> bytes:
    """A binary little-endian PLY of n vertices: xyz (n, 3) float32, rgb (n, 3) uint8; the header is built here, on the host."""
    header, rows = ply_vertices(xyz, rgb)
    return (header + "end_header\n").encode("ascii") + rows


def ply_vertices(xyz: np.ndarray, rgb: np.ndarray) -> Tuple[str, bytes]:
    """The vertex element of this module's PLY and mesh's: the header up to its last property, and the n rows."""
    xyz, rgb = np.asarray(xyz), np.asarray(rgb)
    n = int(xyz.shape[0])
    if xyz.shape != (n, 3) or rgb.shape != (n, 3) or xyz.dtype != np.float32 or rgb.dtype != np.uint8:
        raise ValueError(f"ply_bytes: xyz (n, 3) float32 and rgb (n, 3) uint8, got {xyz.shape} {xyz.dtype} and {rgb.shape} {rgb.dtype}")
    header = ("ply\nformat binary_little_endian 1.0\n" f"element vertex {n}\n"
              "property float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\n")
    rows = np.empty(n, dtype=np.dtype([("xyz", "<f4", 3), ("rgb", "u1", 3)]))
    rows["xyz"], rows["rgb"] = xyz, rgb
    return header, rows.tobytes()


@torch.no_grad()
def reconstruct(model, model_input: Dict, t=(0.0, 1.0), px_tol: float = 1.0, rel_tol: float = 0.01, min_votes: int = 1,
                fuse: bool = True, window: Optional[Sequence[int]] = None) -> PointCloud:
    """The point cloud of the pair(s) in model_input (prepare_pair's dict), in view 0's frame.

    render_path renders the K = len(t) views along the estimated camera path (t = (0, 1): the two photos' own cameras) with
    their depth; vote counts, per pixel, the other views that agree with its depth to px_tol pixels and rel_tol . d; the
    points are formed from depth_fused (fuse=True) or from the depth as rendered.  A pixel is kept iff the depth its point is
    formed from is valid (finite, 0 < d < 10), its votes >= min_votes and forward's `valid_mask` is not zero (the ray meets
    at least one of the two photos); min_votes=0 keeps every valid pixel.  window=(y0, x0, h, w) restricts all views to that
    rectangle of the pixel grid.  Nothing is read on the host here (render_path documents forward's own `pixel_val` copy);
    PointCloud.points is the read."""
    S = int(model_input["context"]["rgb"].shape[2])
    res = render_path(model, model_input, t, window=window, return_rgb=True, return_depth=True)
    return from_views(res, model_input["query"]["intrinsics"], S, px_tol=px_tol, rel_tol=rel_tol, min_votes=min_votes, fuse=fuse,
                      window=window)


@torch.no_grad()
def from_views(views: Dict[str, torch.Tensor], intrinsics: torch.Tensor, S: int, px_tol: float = 1.0, rel_tol: float = 0.01,
               min_votes: int = 1, fuse: bool = True, window: Optional[Sequence[int]] = None) -> PointCloud:
    """reconstruct's second half: the PointCloud of `views`, the dict render_path(..., return_rgb=True, return_depth=True)
    returned for `window` (`depth`, `valid`, `rgb`, `poses`).  Three kernels and the mask between them; no host read."""
    if not 0 <= int(min_votes) <= 255:
        raise ValueError(f"from_views: min_votes must lie in [0, 255], got {min_votes}")
    y0, x0, h, w = (0, 0, int(S), int(S)) if window is None else (int(v) for v in window)
    votes, fused = vote(views["depth"], views["poses"], intrinsics, S, px_tol, rel_tol, window=window)
    depth = fused if fuse else views["depth"]
    xyz = unproject(depth, views["poses"], intrinsics, S, window=window)
    keep = ((depth > 0) & (depth < 10) & (votes >= int(min_votes)) & (views["valid"] != 0)).to(torch.uint8)
    return compact(keep, xyz, views["rgb"], h, w)
