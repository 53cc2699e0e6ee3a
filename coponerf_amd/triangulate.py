"""Two photos in, the 3-D points of their matches out, and the length of the baseline - on the device until the user asks.

`matches` ends at the pose.  Its matches carry sub-pixel, continuous geometry - about 6 000 per pair at stride 4, 131 072 at stride
1 -, and `point_cloud`'s depth map is the depth of one of 2 x 64 samples.  Here

  points        optimal two-view triangulation of every match under a pose: Lindstrom's correction of the match in pixels onto the
                epipolar constraint, then the one point of the two corrected rays; with it both depths, the reprojection error,
                the parallax, a flag byte and - with the photos - a colour: cpn_triangulate_matches, one launch
  depth_scale   the translation's length, which the epipolar residual cannot see: the exact median of (the model's own rendered
                depth of view 0) / (the triangulated depth under |t| = 1), its spread, and the pose head's |t| over it - a verdict
                on the network's translation norm that needs no ground truth: cpn_depth_scale, one launch
  bundle_adjust the pose and one point per match that minimise the reprojection error of both views together, Levenberg-Marquardt
                on the Schur complement of the points, with the Gauss-Newton covariance of the pose and of every point and a
                noise estimate sigma: cpn_bundle_adjust, one launch (round 27)
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

bundle_adjust (round 27): the gauge (|t| = 1, pinned by (tr S / 6) t t^T), sigma = sqrt(2 cost / (rows - 5)), the LM constants (lambda
from 1e-3, / 3 on an accepted step, x 4 on a rejected one, within [1e-12, 1e8]), the stop rule (iters solves, a gain of at most ftol x
cost, lambda > 1e8, a failed solve) and the used-row rule are this package's definitions.  The covariance is the Gauss-Newton one: it
ignores the weights' derivative and the outliers.  On the synthetic scenes its pose is NOT nearer the truth than refine_pose's (the
two costs agree to first order); none of it has been tried on a trained checkpoint.

Left out: feeding the cloud to mesh.integrate, feeding the scale back into Evaluator's columns, a robust (sandwich) covariance, more
workgroups per pair for stride-1 pairs, and tracks over more than two views.
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
def bundle_adjust(tri: Dict[str, torch.Tensor], matches: "_matches.Matches", intrinsics: torch.Tensor, pose: torch.Tensor,
                  inlier: Optional[torch.Tensor] = None, iters: int = 10, scale_px: float = 1.0, ftol: float = 1e-12,
                  min_rows: int = 8) -> Dict[str, torch.Tensor]:
    """cpn_bundle_adjust: tri = points(matches, intrinsics, pose), the same pose (B, 4, 4) fp32, inlier None or (B, N) uint8 ->
    the pose and one point per used row that minimise the robust reprojection error of both views together (refine_pose's cost and
    weight with scale_px, on the 4 pixel residuals of a row), by Levenberg-Marquardt on the Schur complement of the points, at most
    `iters` solves, and their Gauss-Newton covariances.  A row is used iff it is below the count, finite, has flag 0, a non-zero
    inlier byte where given, and starts in front of both cameras.  A dict of `pose` (B, 4, 4) fp32 = [R | |t| of the input times the
    new direction], `xyz` (B, N, 3) fp32, `geom` (B, N, 4) fp32 = (z0, z1, the row's error in pixels, its weight), `cov_x`
    (B, N, 6) fp32, the upper triangle of the point's covariance for unit pixel variance (times sigma^2 for the estimated one),
    `cov` (B, 6, 6) float64, the pose's covariance in (rotation vector, dt) order in the gauge |t| = 1, px^-2 units, and `stats`
    (B, 12) float64: the cost at the start and at the end, the sum of weights, the rows used, steps accepted, rejected, the last
    lambda, sigma = sqrt(2 cost / (rows - 5)), sigma sqrt(tr C_rot) and sigma sqrt(tr C_t) in degrees, the rotation moved in
    degrees, the status (0 ok, 1 a solve failed, 2 not usable: the pose is the input's, everything else NaN).  Rows that are not
    used are NaN.  One launch, one workgroup per pair, float64 inside, nothing read on the host; the workspace (B, 2, N, 3) float64
    is allocated here.  The covariance ignores the weights' derivative and the outliers."""
    named = [("tri['xyz']", tri["xyz"], torch.float32, None), ("tri['flag']", tri["flag"], torch.uint8, None),
             ("matches.xy", matches.xy, torch.float32, None), ("intrinsics", intrinsics, torch.float32, None), ("pose", pose, torch.float32, None)]
    if inlier is not None:
        named.append(("inlier", inlier, torch.uint8, None))
    device_tensors("bundle_adjust", tuple(named))
    B, N = _matches._matches_args("bundle_adjust", matches)
    _matches._cameras("bundle_adjust", intrinsics, pose, B)
    if tuple(tri["xyz"].shape) != (B, N, 3) or tuple(tri["flag"].shape) != (B, N):
        raise ValueError(f"bundle_adjust: tri must be points() of these matches: xyz {(B, N, 3)} and flag {(B, N)}, got "
                         f"{tuple(tri['xyz'].shape)} and {tuple(tri['flag'].shape)}")
    if inlier is not None and tuple(inlier.shape) != (B, N):
        raise ValueError(f"bundle_adjust: inlier must be (B, N) = {(B, N)}, got {tuple(inlier.shape)}")
    if int(iters) < 0 or not 0.0 < float(scale_px) < float("inf") or not 0.0 <= float(ftol) < float("inf") or int(min_rows) < 1:
        raise ValueError(f"bundle_adjust: need iters >= 0, a finite scale_px > 0, a finite ftol >= 0 and min_rows >= 1, got {iters}, "
                         f"{scale_px}, {ftol}, {min_rows}")
    if not 1 <= B <= 32767 or N > 2 ** 24:
        raise ValueError(f"bundle_adjust: need 1 <= B <= 32767 and N <= 2^24, got B = {B}, N = {N}")
    dev = matches.xy.device
    work = torch.empty(B, 2, N, 3, dtype=torch.float64, device=dev)
    out = {"pose": torch.empty(B, 4, 4, dtype=torch.float32, device=dev), "xyz": torch.empty(B, N, 3, dtype=torch.float32, device=dev),
           "geom": torch.empty(B, N, 4, dtype=torch.float32, device=dev), "cov_x": torch.empty(B, N, 6, dtype=torch.float32, device=dev),
           "cov": torch.empty(B, 6, 6, dtype=torch.float64, device=dev),
           "stats": torch.empty(B, _hip.CONSTANTS["BUNDLE_STATS"], dtype=torch.float64, device=dev)}
    with torch.cuda.device(dev):
        _hip.call("cpn_bundle_adjust", matches.xy.data_ptr(), matches.count.data_ptr(), intrinsics.data_ptr(), pose.data_ptr(),
                  tri["xyz"].data_ptr(), tri["flag"].data_ptr(), inlier.data_ptr() if inlier is not None else None, B, N, int(iters),
                  float(scale_px), float(ftol), int(min_rows), work.data_ptr(), out["pose"].data_ptr(), out["xyz"].data_ptr(),
                  out["geom"].data_ptr(), out["cov_x"].data_ptr(), out["cov"].data_ptr(), out["stats"].data_ptr(), _hip.stream_handle())
    return out


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
          inlier: Optional[torch.Tensor] = None, max_rel_sigma_z: Optional[float] = None, cov_x: Optional[torch.Tensor] = None,
          sigma: Optional[torch.Tensor] = None) -> "point_cloud.PointCloud":
    """The PointCloud of points()' dict: a row is kept iff its flag is 0, its reprojection error is at most max_reproj_px, its
    parallax at least min_parallax_deg and, with inlier (B, N) (ransac_pose's mask), inlier is not zero.  Stock ops form the mask,
    point_cloud.compact (K = 1, h = 1, w = N) compacts it: the kept rows in the matches' order, no new kernel, nothing read on
    the host.  Without colours in tri the points are grey.  max_rel_sigma_z: with bundle_adjust's `cov_x` (B, N, 6) and a `sigma`
    (B) - its stats[:, 7] - a row is also dropped unless sigma sqrt(cov_zz) / z0 <= max_rel_sigma_z (a NaN drops it); without the
    keyword the mask and the bytes are as before."""
    xyz, geom, flag = tri["xyz"], tri["geom"], tri["flag"]
    B, N = int(flag.shape[0]), int(flag.shape[1])
    keep = (flag == 0) & (geom[..., 2] <= float(max_reproj_px)) & (geom[..., 3] >= float(min_parallax_deg))
    if inlier is not None:
        if tuple(inlier.shape) != (B, N) or inlier.device != flag.device:
            raise ValueError(f"cloud: inlier must be (B, N) = {(B, N)} on tri's device, got {tuple(inlier.shape)}")
        keep &= inlier != 0
    if max_rel_sigma_z is not None:
        if cov_x is None or sigma is None or tuple(cov_x.shape) != (B, N, 6) or tuple(sigma.shape) != (B,):
            raise ValueError(f"cloud: max_rel_sigma_z needs cov_x (B, N, 6) and sigma (B) with (B, N) = {(B, N)}")
        keep &= sigma.double()[:, None] * cov_x[..., 5].double().sqrt() / geom[..., 0].double() <= float(max_rel_sigma_z)
    rgb = tri["rgb"] if "rgb" in tri else torch.zeros_like(xyz)
    return point_cloud.compact(keep.to(torch.uint8)[None].contiguous(), xyz[None], rgb[None], 1, N)


@torch.no_grad()
def from_pair(model, model_input: Dict, pose: str = "selected", scale: str = "given", max_reproj_px: float = 1.0,
              min_parallax_deg: float = 1.0, min_rows: int = 8, inliers_only: bool = False, adjust: Optional[Dict] = None,
              **matches_keywords) -> Dict:
    """The triangulated cloud of the pair(s) in model_input (prepare_pair's dict).  matches.from_pair runs (get_z once; its
    keywords - S, stride, max_cycle_px, ransac, select, .. - are handed on); the matches are triangulated under `pose`: "network"
    (get_z's rel_pose), "refined" (refine_pose's), "ransac" (ransac_pose's; ransac={} is added where the keyword is missing) or
    "selected" (select_pose's, likewise).  scale="given" takes the pose's translation as it is - the network's length, whatever the
    estimator -; scale="depth" triangulates under |t| = 1, renders view 0's depth ONCE (render_path at t = 0, which runs get_z
    again), takes depth_scale against it, rescales the pose and triangulates again: two more launches and the render.
    inliers_only=True keeps ransac_pose's inliers alone (pose "ransac" or "selected").  adjust: None, or a dict of bundle_adjust's
    keywords (iters, scale_px, ftol, min_rows) and cloud's max_rel_sigma_z: bundle_adjust runs after the last points call (on the
    inliers alone with inliers_only), the cloud is formed from the adjusted points - with the error and the flags of the adjusted
    rows: a row that bundle_adjust did not use is dropped - and the result gains the key `adjust`, its dict; `pose` stays the pose
    the triangulation used.  Without the keyword nothing is launched.
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
    if adjust is not None:
        if not isinstance(adjust, dict) or set(adjust) - {"iters", "scale_px", "ftol", "min_rows", "max_rel_sigma_z"}:
            raise ValueError(f"from_pair: adjust must be None or a dict of iters, scale_px, ftol, min_rows and max_rel_sigma_z, got {adjust!r}")
        adjust_kw = dict(adjust)
        max_rel_sigma_z = adjust_kw.pop("max_rel_sigma_z", None)
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
    result = {"pose": chosen, "scale": None if ds is None else ds["scale"], "stats": None if ds is None else ds["stats"], "points": tri,
              "matches": found}
    if adjust is None:
        result["cloud"] = cloud(tri, max_reproj_px=max_reproj_px, min_parallax_deg=min_parallax_deg, inlier=inlier)
        return result
    ba = result["adjust"] = bundle_adjust(tri, m, intrinsics, chosen, inlier=inlier, **adjust_kw)
    moved = dict(tri)                                                   # the adjusted points; the parallax stays round 26's
    moved["xyz"] = ba["xyz"]
    moved["geom"] = torch.cat((ba["geom"][..., :3], tri["geom"][..., 3:]), dim=-1)
    moved["flag"] = torch.where(torch.isnan(ba["xyz"][..., 2]), torch.full_like(tri["flag"], 255), tri["flag"])
    result["cloud"] = cloud(moved, max_reproj_px=max_reproj_px, min_parallax_deg=min_parallax_deg, inlier=inlier,
                            max_rel_sigma_z=max_rel_sigma_z, cov_x=ba["cov_x"], sigma=ba["stats"][:, 7])
    return result
