"""Two photos in, the 3-D points of their matches out, and the length of the baseline - on the device until the user asks.

`matches` ends at the pose.  Its matches carry sub-pixel, continuous geometry - about 6 000 per pair at stride 4, 131 072 at stride
1 -, and `point_cloud`'s depth map is the depth of one of 2 x 64 samples.  Here

  points        optimal two-view triangulation of every match under a pose: Lindstrom's correction of the match in pixels onto the
                epipolar constraint, then the one point of the two corrected rays; with it both depths, the reprojection error,
                the parallax, a flag byte and - with the photos - a colour: cpn_triangulate_matches, one launch
  depth_scale   the translation's length, which the epipolar residual cannot see: the exact median of (the model's own rendered
                depth of view 0) / (the triangulated depth under |t| = 1), its spread, and the pose head's |t| over it - a verdict
                on the network's translation norm that needs no ground truth: cpn_depth_scale, one launch
  rescale       [R | scale t / |t|] by torch.where
  cloud         the kept points as a point_cloud.PointCloud (save, points(b), frames and splat.draw work on it unchanged)
  from_pair     matches.from_pair, points under the chosen pose and, with scale="depth", one render of view 0's depth, depth_scale,
                rescale and points again

The conventions and the arithmetic are in include/coponerf_hip.h (round 26): X0 = R X1 + t, the points are in view 0's frame, t is
used as given.  The pass count (CPN_TRIANGULATE_PASSES = 3: within 1e-15 px of convergence on a match within 2 px of the constraint,
within 0.03 px on a 176 px outlier that no keep rule takes), the keep rule (flag 0, reprojection error <= max_reproj_px = 1 pixel,
parallax >= min_parallax_deg = 1 degree) and its defaults, the nearest-pixel read of the depth map and the median rule (the lower
middle, round 25's rank rule) are this package's definitions.  None of it has been tried on a trained checkpoint, because none is
available offline; on the synthetic weights the flows carry no geometry, and the cloud is empty or tiny.

Left out: two-view bundle adjustment over points and pose, per-point covariances, feeding the cloud to mesh.integrate, feeding the
scale back into Evaluator's columns, and tracks over more than two views.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import _hip
from . import matches as _matches
from . import point_cloud
from ._args import device_tensors

FLAGS = {"input": _hip.CONSTANTS["TRI_INPUT"], "correction": _hip.CONSTANTS["TRI_CORRECTION"], "parallax": _hip.CONSTANTS["TRI_PARALLAX"],
         "behind0": _hip.CONSTANTS["TRI_BEHIND0"], "behind1": _hip.CONSTANTS["TRI_BEHIND1"]}
_POSES = ("selected", "network", "refined", "ransac")
_SCALES = ("given", "depth")


@torch.no_grad()
def points(matches: "_matches.Matches", intrinsics: torch.Tensor, pose: torch.Tensor, images: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """cpn_triangulate_matches: the Matches of B pairs, intrinsics (B, 2, 4, 4) fp32 (`context.intrinsics`), pose (B, 4, 4) fp32 with
    X0 = R X1 + t, images None or (B, 2, S, S, 3) fp32 in [-1, 1] (`context.rgb`) -> a dict of `xyz` (B, N, 3) fp32, the points in
    view 0's frame; `geom` (B, N, 4) fp32 = (z0, z1, the reprojection error sqrt(|D|^2 + |D'|^2) in pixels, the parallax in
    degrees); `flag` (B, N) uint8, the bits of FLAGS: 1 a row or a pose that is not finite (or t = 0), 2 the correction failed
    (disc < 0 or a zero denominator: a match on both epipoles), 4 no parallax, 8 z0 <= 0, 16 z1 <= 0, 255 at and beyond the count
    (those rows are NaN); and with images `rgb` (B, N, 3) fp32 in [-1, 1], the bilinear samples of both photos at the match,
    averaged.  One launch, one thread per (pair, row), float64 inside, nothing read on the host.  t is used as given: the points
    scale with it."""
    xy, count = matches.xy, matches.count
    named = [("matches.xy", xy, torch.float32, None), ("intrinsics", intrinsics, torch.float32, None), ("pose", pose, torch.float32, None)]
    if images is not None:
        named.append(("images", images, torch.float32, None))
    device_tensors("points", tuple(named))
    B, N = _matches._matches_args("points", matches)
    _matches._cameras("points", intrinsics, pose, B)
    S = 0
    if images is not None:
        if images.dim() != 5 or tuple(images.shape[:2]) != (B, 2) or images.shape[2] != images.shape[3] or images.shape[4] != 3:
            raise ValueError(f"points: images must be (B, 2, S, S, 3) with B = {B} (`context.rgb`), got {tuple(images.shape)}")
        S = int(images.shape[2])
    if not 1 <= B <= 32767 or N > 2 ** 24 or S > 16384:
        raise ValueError(f"points: need 1 <= B <= 32767, N <= 2^24 and S <= 16384, got B = {B}, N = {N}, S = {S}")
    dev = xy.device
    out = {"xyz": torch.empty(B, N, 3, dtype=torch.float32, device=dev), "geom": torch.empty(B, N, 4, dtype=torch.float32, device=dev),
           "flag": torch.empty(B, N, dtype=torch.uint8, device=dev)}
    if images is not None:
        out["rgb"] = torch.empty(B, N, 3, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _hip.call("cpn_triangulate_matches", xy.data_ptr(), count.data_ptr(), intrinsics.data_ptr(), pose.data_ptr(),
                  images.data_ptr() if images is not None else None, B, N, S, out["xyz"].data_ptr(), out["geom"].data_ptr(),
                  out["flag"].data_ptr(), out["rgb"].data_ptr() if images is not None else None, _hip.stream_handle())
    return out


@torch.no_grad()
def depth_scale(tri: Dict[str, torch.Tensor], matches: "_matches.Matches", depth0: torch.Tensor, S: int, rel_pose: Optional[torch.Tensor] = None,
                max_reproj_px: float = 1.0, min_parallax_deg: float = 1.0, min_rows: int = 8) -> Dict[str, torch.Tensor]:
    """cpn_depth_scale: tri = points(matches, intrinsics, a pose with |t| = 1), depth0 (B, S S) fp32 a z-depth map of view 0 on the
    S x S grid of the matches (render_path(..., [0.0], return_depth=True)["depth"][0]) -> `scale` (B) float64, the exact lower
    median of q = depth0 at the NEAREST pixel of (x0, y0) over z0, over the rows with flag 0, an error <= max_reproj_px, a parallax
    >= min_parallax_deg and a valid depth (finite, 0 < d < 10: point_cloud's rule), and `stats` (B, 4) float64: the rows used, the
    exact median of |q / scale - 1|, |t| of rel_pose over scale (NaN without one), the status (0 ok, 1 fewer than min_rows rows:
    scale is NaN).  One launch, one workgroup per pair, nothing read on the host; the order statistics are round 25's radix
    descent.  [2] near 1 says that the pose head's translation norm agrees with the depth the model renders."""
    named = [("tri['geom']", tri["geom"], torch.float32, None), ("tri['flag']", tri["flag"], torch.uint8, None),
             ("matches.xy", matches.xy, torch.float32, None), ("depth0", depth0, torch.float32, None)]
    if rel_pose is not None:
        named.append(("rel_pose", rel_pose, torch.float32, None))
    device_tensors("depth_scale", tuple(named))
    B, N = _matches._matches_args("depth_scale", matches)
    S = int(S)
    if tuple(tri["geom"].shape) != (B, N, 4) or tuple(tri["flag"].shape) != (B, N):
        raise ValueError(f"depth_scale: tri must be points() of these matches: geom {(B, N, 4)} and flag {(B, N)}, got "
                         f"{tuple(tri['geom'].shape)} and {tuple(tri['flag'].shape)}")
    if not 1 <= S <= 16384 or tuple(depth0.shape) != (B, S * S):
        raise ValueError(f"depth_scale: depth0 must be (B, S S) with B = {B} and 1 <= S = {S} <= 16384, got {tuple(depth0.shape)}")
    if rel_pose is not None and tuple(rel_pose.shape) != (B, 4, 4):
        raise ValueError(f"depth_scale: rel_pose must be (B, 4, 4) with B = {B}, got {tuple(rel_pose.shape)}")
    if not (0.0 <= float(max_reproj_px) < float("inf") and 0.0 <= float(min_parallax_deg) < float("inf")) or int(min_rows) < 1:
        raise ValueError(f"depth_scale: need finite max_reproj_px, min_parallax_deg >= 0 and min_rows >= 1, got {max_reproj_px}, "
                         f"{min_parallax_deg}, {min_rows}")
    if not 1 <= B <= 32767 or N > 2 ** 24:
        raise ValueError(f"depth_scale: need 1 <= B <= 32767 and N <= 2^24, got B = {B}, N = {N}")
    dev = matches.xy.device
    scale = torch.empty(B, dtype=torch.float64, device=dev)
    stats = torch.empty(B, 4, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _hip.call("cpn_depth_scale", tri["geom"].data_ptr(), tri["flag"].data_ptr(), matches.xy.data_ptr(), matches.count.data_ptr(),
                  depth0.data_ptr(), rel_pose.data_ptr() if rel_pose is not None else None, B, N, S, float(max_reproj_px),
                  float(min_parallax_deg), int(min_rows), scale.data_ptr(), stats.data_ptr(), _hip.stream_handle())
    return {"scale": scale, "stats": stats}


@torch.no_grad()
def rescale(pose: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """[R | scale t / |t|] of pose (B, 4, 4) fp32 and scale (B) - the direction and the product in float64, rounded to fp32 once -
    by torch.where: a pair whose scale or whose new translation is not finite (depth_scale's status 1, t = 0) keeps its pose."""
    t = pose[:, :3, 3].double()
    new = scale.double()[:, None] * (t / t.norm(dim=1, keepdim=True))
    ok = torch.isfinite(new).all(dim=1, keepdim=True)
    out = pose.clone()
    out[:, :3, 3] = torch.where(ok, new.float(), pose[:, :3, 3])
    return out


@torch.no_grad()
def cloud(tri: Dict[str, torch.Tensor], max_reproj_px: float = 1.0, min_parallax_deg: float = 1.0,
          inlier: Optional[torch.Tensor] = None) -> "point_cloud.PointCloud":
    """The PointCloud of points()' dict: a row is kept iff its flag is 0, its reprojection error is at most max_reproj_px, its
    parallax at least min_parallax_deg and, with inlier (B, N) (ransac_pose's mask), inlier is not zero.  Stock ops form the mask,
    point_cloud.compact (K = 1, h = 1, w = N) compacts it: the kept rows in the matches' order, no new kernel, nothing read on
    the host.  Without colours in tri the points are grey."""
    xyz, geom, flag = tri["xyz"], tri["geom"], tri["flag"]
    B, N = int(flag.shape[0]), int(flag.shape[1])
    keep = (flag == 0) & (geom[..., 2] <= float(max_reproj_px)) & (geom[..., 3] >= float(min_parallax_deg))
    if inlier is not None:
        if tuple(inlier.shape) != (B, N) or inlier.device != flag.device:
            raise ValueError(f"cloud: inlier must be (B, N) = {(B, N)} on tri's device, got {tuple(inlier.shape)}")
        keep &= inlier != 0
    rgb = tri["rgb"] if "rgb" in tri else torch.zeros_like(xyz)
    return point_cloud.compact(keep.to(torch.uint8)[None].contiguous(), xyz[None], rgb[None], 1, N)


@torch.no_grad()
def from_pair(model, model_input: Dict, pose: str = "selected", scale: str = "given", max_reproj_px: float = 1.0,
              min_parallax_deg: float = 1.0, min_rows: int = 8, inliers_only: bool = False, **matches_keywords) -> Dict:
    """The triangulated cloud of the pair(s) in model_input (prepare_pair's dict).  matches.from_pair runs (get_z once; its
    keywords - S, stride, max_cycle_px, ransac, select, .. - are handed on); the matches are triangulated under `pose`: "network"
    (get_z's rel_pose), "refined" (refine_pose's), "ransac" (ransac_pose's; ransac={} is added where the keyword is missing) or
    "selected" (select_pose's, likewise).  scale="given" takes the pose's translation as it is - the network's length, whatever the
    estimator -; scale="depth" triangulates under |t| = 1, renders view 0's depth ONCE (render_path at t = 0, which runs get_z
    again), takes depth_scale against it, rescales the pose and triangulates again: two more launches and the render.
    inliers_only=True keeps ransac_pose's inliers alone (pose "ransac" or "selected").
    -> `cloud` (a PointCloud, coloured from the two photos), `pose` (B, 4, 4) the pose the points were formed under, `scale` (B)
    float64 and `stats` (B, 4) float64 (depth_scale's; None with scale="given"), `points` (points()' dict) and `matches`
    (matches.from_pair's dict).  Nothing is read on the host; PointCloud.points is the read.  On the synthetic weights the flows
    carry no geometry: the cloud is empty or tiny, and that only shows that the path runs."""
    if pose not in _POSES:
        raise ValueError(f"from_pair: pose must be one of {_POSES}, got {pose!r}")
    if scale not in _SCALES:
        raise ValueError(f"from_pair: scale must be one of {_SCALES}, got {scale!r}")
    if inliers_only and pose not in ("ransac", "selected"):
        raise ValueError(f"from_pair: inliers_only needs pose \"ransac\" or \"selected\", got {pose!r}")
    kw = dict(matches_keywords)
    if pose == "ransac":
        kw.setdefault("ransac", {})
    if pose == "selected":
        kw.setdefault("select", {})
    kw["refine"] = pose == "refined" or bool(kw.get("refine", False))
    found = _matches.from_pair(model, model_input, **kw)
    chosen = {"network": lambda: found["rel_pose"], "refined": lambda: found["pose"], "ransac": lambda: found["ransac"]["pose"],
              "selected": lambda: found["select"]["pose"]}[pose]().contiguous()
    inlier = None
    if inliers_only:
        inlier = found["ransac"]["inlier"] if pose == "ransac" else found["select"]["ransac"]["inlier"]
    ctx = model_input["context"]
    intrinsics, images = ctx["intrinsics"].float().contiguous(), ctx["rgb"].float().contiguous()
    m = found["matches"]
    ds = None
    S = int(kw.get("S", 256))
    if int(images.shape[2]) != S:                                       # the photos are not on the matches' grid: grey points
        images = None
        if scale == "depth":
            raise ValueError(f"from_pair: scale=\"depth\" renders view 0 on the photos' grid, which must be the matches' (S = {S}), got "
                             f"{tuple(ctx['rgb'].shape)}")
    if scale == "depth":
        from .novel_views import render_path
        unit = rescale(chosen, torch.ones(chosen.shape[0], dtype=torch.float64, device=chosen.device))
        first = points(m, intrinsics, unit)
        depth0 = render_path(model, model_input, (0.0,), return_depth=True)["depth"][0].contiguous()
        ds = depth_scale(first, m, depth0, S, rel_pose=found["rel_pose"].contiguous(), max_reproj_px=max_reproj_px,
                         min_parallax_deg=min_parallax_deg, min_rows=min_rows)
        chosen = rescale(chosen, ds["scale"])
    tri = points(m, intrinsics, chosen, images)
    return {"cloud": cloud(tri, max_reproj_px=max_reproj_px, min_parallax_deg=min_parallax_deg, inlier=inlier), "pose": chosen,
            "scale": None if ds is None else ds["scale"], "stats": None if ds is None else ds["stats"], "points": tri, "matches": found}
