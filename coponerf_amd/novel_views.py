"""Two photos in, views in between out: what a user with a checkpoint does after `test.py`, kept on the device.

The reference has no script for it.  By hand it takes the loader's whole contract (a nested dict of float images at exactly
256 x 256, 4 x 4 intrinsics in the loader's units, a `uv` grid), camera-to-world matrices the user does not have - the method
is pose-free -, a Python loop over `forward` and a float -> uint8 round trip per frame on the host.  Here

  prepare_pair   two uint8 photos of any size (host or device) -> the model's input dict: cpn_fit_images_u8         dataio.py:340-353,
                 (centre square crop, resample, normalise) and the intrinsics that follow the crop and the scale    data_util.py:116-121
  camera_path    K cameras between view 0 and the ESTIMATED view 1: cpn_camera_path reads rel_pose on the device    test.py:96-121
  render_path    get_z once, one forward(val=True) per camera with the next camera announced under the current     CoPoNeRF.py:240-242
                 render (CoPoNeRF.prepare_next), cpn_pack_frames writes each frame into the uint8 output

`forward(val=True)` renders through the estimated pose (models/CoPoNeRF.py:240-242: view 1's camera is rel_pose, view 0's the
identity), so the path needs no pose from the user and no kernel of the render path changes.  The ground-truth entries of the
outputs (`gt_rel_pose`, `gt_rel_pose_flip`) are formed from the identity matrices prepare_pair fills in and mean nothing here.
"""
from __future__ import annotations

import math
import warnings
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _hip
from .shards import crop_window
from .summaries import _jet_on


# -------------------------------------------------------------------------------------------------------------- the pair
def fit_intrinsics(K_px, Hi: int, Wi: int, size: int) -> np.ndarray:
    """(4, 4) float64: the model's intrinsics of a photo of Hi x Wi pixels with pixel intrinsics K_px (3, 3) after the centre
    square crop and the resample to size x size: diag(s, s, 1) . (K_px shifted by the crop's offset), s = size / side.  The
    offset is the centred one, ((Wi - side) / 2, (Hi - side) / 2): a principal point at the photo's centre stays at the
    centre as in the loader (dataio.py:343-348; shards.sample_intrinsics), also where the margin is odd and the crop
    window itself starts half a pixel beside it."""
    K_px = np.asarray(K_px, dtype=np.float64)
    if K_px.shape != (3, 3):
        raise ValueError(f"fit_intrinsics: K_px must be (3, 3), got {K_px.shape}")
    _, _, side = crop_window(Hi, Wi)
    s = size / side
    K = K_px.copy()
    K[0, 2] -= (Wi - side) / 2.0
    K[1, 2] -= (Hi - side) / 2.0
    K[:2] *= s
    out = np.eye(4, dtype=np.float64)
    out[:3, :3] = K
    return out


def hfov_intrinsics(hfov_deg: float, Hi: int, Wi: int) -> np.ndarray:
    """(3, 3) float64 pixel intrinsics of a photo with horizontal field of view hfov_deg, square pixels and the principal
    point at the centre."""
    if not 0.0 < float(hfov_deg) < 180.0:
        raise ValueError(f"hfov_deg must lie in (0, 180), got {hfov_deg}")
    f = 0.5 * Wi / math.tan(math.radians(float(hfov_deg)) / 2.0)
    return np.array([[f, 0.0, Wi / 2.0], [0.0, f, Hi / 2.0], [0.0, 0.0, 1.0]])


def _as_u8_batch(name: str, img) -> torch.Tensor:
    t = img
    if isinstance(img, np.ndarray):
        with warnings.catch_warnings():                     # a read-only array is fine: the image is only read
            warnings.simplefilter("ignore", UserWarning)
            t = torch.from_numpy(np.ascontiguousarray(img))
    if not torch.is_tensor(t):
        raise TypeError(f"prepare_pair: {name} must be a torch tensor or a numpy array")
    if t.dtype != torch.uint8:
        raise ValueError(f"prepare_pair: uint8 images only, {name} is {t.dtype}")
    if t.dim() == 3:
        t = t.unsqueeze(0)
    if t.dim() != 4 or t.shape[3] != 3 or t.shape[1] < 2 or t.shape[2] < 2:
        raise ValueError(f"prepare_pair: {name} must be (Hi, Wi, 3) or (B, Hi, Wi, 3) of at least 2 x 2, got {tuple(t.shape)}")
    return t.contiguous()


def _per_view(name: str, value, B: int, tail: Tuple[int, ...]) -> np.ndarray:
    """value broadcast to (B, 2) + tail in float64: one for both views, one per view, or one per pair and view."""
    a = np.asarray(value.detach().cpu() if torch.is_tensor(value) else value, dtype=np.float64)
    nt = len(tail)
    if a.shape[a.ndim - nt:] != tail or a.ndim - nt > 2:
        raise ValueError(f"prepare_pair: {name} must end in {tail} with at most (B, 2) in front, got {a.shape}")
    lead = a.shape[:a.ndim - nt]
    if lead == ():
        a = a[None, None]
    elif lead == (2,):
        a = a[None]
    elif len(lead) != 2 or lead[1] != 2 or lead[0] not in (1, B):
        raise ValueError(f"prepare_pair: {name}: one value, one per view (2, ...) or one per pair and view (B, 2, ...), got {a.shape}")
    return np.broadcast_to(a, (B, 2) + tail)


_UV: Dict[Tuple[torch.device, int], torch.Tensor] = {}


def _uv_grid(S: int, dev: torch.device) -> torch.Tensor:
    """(S * S, 2) fp32 on the device: the full pixel grid, row-major, (x = column, y = row)."""
    g = _UV.get((dev, S))
    if g is None:
        a = torch.arange(S, dtype=torch.float32, device=dev)
        g = _UV[(dev, S)] = torch.stack((a.repeat(S), a.repeat_interleave(S)), dim=-1).contiguous()
    return g


@torch.no_grad()
def fit_images(view0: torch.Tensor, view1: torch.Tensor, out: torch.Tensor, antialias: bool = True) -> None:
    """cpn_fit_images_u8 on the two views of B pairs: view_v (B, Hi_v, Wi_v, 3) uint8 on the host or the device ->
    out[:, v] of out (B, 2, size, size, 3) fp32 on the device.  Host views go through ONE pinned staging buffer and one
    asynchronous copy; two views of one size share one launch."""
    dev = out.device
    B, size = int(out.shape[0]), int(out.shape[2])
    views = [view0, view1]
    host = [v for v in views if not v.is_cuda]
    if host:
        stage = torch.empty(sum(v.numel() for v in host), dtype=torch.uint8, pin_memory=True)
        at = 0
        for v in host:
            stage[at:at + v.numel()].copy_(v.reshape(-1))
            at += v.numel()
        pieces = iter(stage.to(dev, non_blocking=True).split([v.numel() for v in host]))
    flat = [v.reshape(-1) if v.is_cuda else next(pieces) for v in views]
    SS3 = size * size * 3
    if view0.shape == view1.shape:                          # one launch: image n = v B + b
        one = flat[1].untyped_storage().data_ptr() == flat[0].untyped_storage().data_ptr() and \
            flat[1].storage_offset() == flat[0].storage_offset() + flat[0].numel()
        launches = [(flat[0] if one else torch.cat(flat), 0, 2 * B, view0.shape)]
    else:
        launches = [(flat[0], 0, B, view0.shape), (flat[1], 1, B, view1.shape)]
    with torch.cuda.device(dev):
        for src, v, N, shape in launches:
            Hi, Wi = int(shape[1]), int(shape[2])
            tmp = torch.empty(N * size * crop_window(Hi, Wi)[2] * 3, dtype=torch.float32, device=dev)
            _hip.call("cpn_fit_images_u8", src.data_ptr(), N, B, Hi, Wi, size, 1 if antialias else 0, tmp.data_ptr(),
                      out.data_ptr() + 4 * v * SS3, 2 * SS3, SS3, _hip.stream_handle())


@torch.no_grad()
def prepare_pair(img0, img1, intrinsics=None, hfov_deg=None, size: int = 256, antialias: bool = True,
                 device: Optional[torch.device] = None) -> Dict:
    """The model's input dict of two photos.

    img0, img1   uint8 (Hi, Wi, 3) or (B, Hi, Wi, 3), torch tensors or numpy arrays, on the host or the device; each view may
                 have its own size.  Host images are staged through pinned memory and uploaded with one asynchronous copy.
    intrinsics   (3, 3) in pixels of the ORIGINAL photo: one for both views, (2, 3, 3) per view or (B, 2, 3, 3).
    hfov_deg     instead of intrinsics: the horizontal field of view in degrees (one, (2,) per view or (B, 2)), square pixels,
                 principal point at the centre.  Exactly one of the two is given.
    size         side of the model's images; get_z is built for 256.
    antialias    True: F.interpolate(mode="bilinear", antialias=True, align_corners=False) of the cropped photo, which
                 averages over the footprint of an output pixel when the photo is larger.  False: the same operator with
                 antialias=False, the half-pixel two-tap bilinear formula cv2.resize applies to the loader's 360-row frames -
                 in float: cv2's 11-bit fixed-point weights are not reproduced.

    The images are normalised as `v / 127.5 - 1` on the fp32 resampled value v, which is never rounded back to a byte: up to
    half a grey level more exact than the loader, which resizes to uint8 first.  A photo whose crop already is size x size
    gets exactly the loader's values.  The intrinsics are formed in float64 (fit_intrinsics) and rounded to fp32 once.

    Returns the reference's input dict on the device: context.rgb (B, 2, size, size, 3), context.intrinsics (B, 2, 4, 4),
    context.cam2world two identities; query: the full row-major uv grid (B, 1, size^2, 2) (x = column, y = row), the identity
    as cam2world, view 0's intrinsics and a zero rgb.  There are no true poses in it: `gt_rel_pose` and `gt_rel_pose_flip`
    of the model's outputs are then meaningless (the identity)."""
    if (intrinsics is None) == (hfov_deg is None):
        raise ValueError("prepare_pair: give exactly one of intrinsics and hfov_deg")
    views = [_as_u8_batch("img0", img0), _as_u8_batch("img1", img1)]
    B = int(views[0].shape[0])
    if int(views[1].shape[0]) != B:
        raise ValueError(f"prepare_pair: {B} first and {int(views[1].shape[0])} second images")
    size = int(size)
    if size < 1:
        raise ValueError(f"prepare_pair: size must be positive, got {size}")
    on_dev = [t.device for t in views if t.is_cuda]
    dev = torch.device(device) if device is not None else (on_dev[0] if on_dev else torch.device("cuda", torch.cuda.current_device()))
    if dev.type != "cuda" or any(d != dev for d in on_dev):
        raise RuntimeError("prepare_pair runs on one HIP device (coponerf_amd has no non-HIP compute path)")

    K = np.empty((B, 2, 4, 4), dtype=np.float64)
    if intrinsics is not None:
        Kpx = _per_view("intrinsics", intrinsics, B, (3, 3))
    else:
        fov = _per_view("hfov_deg", hfov_deg, B, ())
    for v in range(2):
        Hi, Wi = int(views[v].shape[1]), int(views[v].shape[2])
        for b in range(B):
            K[b, v] = fit_intrinsics(Kpx[b, v] if intrinsics is not None else hfov_intrinsics(fov[b, v], Hi, Wi), Hi, Wi, size)
    # the four small tensors of the dict, each contiguous, in one pinned buffer and one upload
    K32 = torch.from_numpy(K.astype(np.float32))
    eye = torch.eye(4, dtype=torch.float32)
    parts = (K32, eye.expand(B, 2, 4, 4), K32[:, :1], eye.expand(B, 1, 4, 4))
    small = torch.empty(sum(p.numel() for p in parts), dtype=torch.float32, pin_memory=True)
    at = 0
    for p in parts:
        small[at:at + p.numel()] = p.reshape(-1)
        at += p.numel()
    small = small.to(dev, non_blocking=True)
    ctx_K, ctx_c2w, qry_K, qry_c2w = (m.view(B, -1, 4, 4) for m in small.split([p.numel() for p in parts]))

    ctx = torch.empty(B, 2, size, size, 3, dtype=torch.float32, device=dev)
    fit_images(views[0], views[1], ctx, antialias)
    R = size * size
    context = {"rgb": ctx, "cam2world": ctx_c2w, "intrinsics": ctx_K}
    query = {"rgb": torch.zeros(B, 1, R, 3, dtype=torch.float32, device=dev), "cam2world": qry_c2w, "intrinsics": qry_K,
             "uv": _uv_grid(size, dev).expand(B, 1, R, 2).contiguous()}
    return {"query": query, "context": context}


# -------------------------------------------------------------------------------------------------------------- the path
@torch.no_grad()
def camera_path(rel_pose: torch.Tensor, t, sway: float = 0.0, turns: float = 2.0) -> torch.Tensor:
    """(K, B, 4, 4) fp32 on the device: pose k is the virtual camera t[k] of the way from view 0 to view 1, in view 0's frame -
    what `query.cam2world` holds when view 0's cam2world is the identity.  Rotation exp(t log R_rel), position t t_rel;
    t outside [0, 1] extrapolates, t == 0 is the identity and t == 1 rel_pose itself.  sway > 0 adds
    sway (cos(2 pi turns t), sin(2 pi turns t), 0) in the camera's own frame (test.py's make_circle).
    rel_pose (B, 4, 4) fp32 stays on the device (cpn_camera_path; float64 inside); t: K numbers or a tensor of K."""
    if not torch.is_tensor(rel_pose) or not rel_pose.is_cuda:
        raise RuntimeError("camera_path runs on the HIP device only (coponerf_amd has no non-HIP compute path)")
    if rel_pose.dim() != 3 or rel_pose.shape[1:] != (4, 4) or rel_pose.dtype != torch.float32:
        raise ValueError(f"camera_path: rel_pose must be (B, 4, 4) fp32, got {tuple(rel_pose.shape)} {rel_pose.dtype}")
    if not float(sway) >= 0.0:
        raise ValueError(f"camera_path: sway must be >= 0, got {sway}")
    dev = rel_pose.device
    if torch.is_tensor(t) and t.is_cuda:
        td = t.to(device=dev, dtype=torch.float64).reshape(-1).contiguous()
    else:
        th = torch.as_tensor(t, dtype=torch.float64).reshape(-1)
        td = torch.empty(th.numel(), dtype=torch.float64, pin_memory=True).copy_(th).to(dev, non_blocking=True)
    K, B = int(td.numel()), int(rel_pose.shape[0])
    if K < 1 or B < 1:
        raise ValueError(f"camera_path: need at least one t and one pair, got K = {K}, B = {B}")
    rel = rel_pose.contiguous()
    out = torch.empty(K, B, 4, 4, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _hip.call("cpn_camera_path", rel.data_ptr(), td.data_ptr(), B, K, float(sway), float(turns), out.data_ptr(),
                  _hip.stream_handle())
    return out


# ------------------------------------------------------------------------------------------------------------ the frames
@torch.no_grad()
def pack_frames(rgb: torch.Tensor, out: torch.Tensor, depth: Optional[torch.Tensor] = None) -> torch.Tensor:
    """cpn_pack_frames: rgb (B, ..., h * w, 3) fp32 in [-1, 1] -> out (B, h, w, 3) uint8 =
    rint(min(max((x + 1) * 127.5, 0), 255)), NaN -> 0; with depth (B, h * w[, 1]) fp32, out is (B, h, 2 w, 3) and its right half
    matplotlib's `jet` of depth / 10 (summaries.depth_colors) times 255, rounded alike.  out may be a frame of a larger tensor."""
    if out.dtype != torch.uint8 or out.dim() != 4 or out.shape[3] != 3 or not out.is_contiguous() or not out.is_cuda:
        raise ValueError(f"pack_frames: out must be a contiguous (B, h, w', 3) uint8 device tensor, got {tuple(out.shape)} {out.dtype}")
    B, h, wo = int(out.shape[0]), int(out.shape[1]), int(out.shape[2])
    w = wo // 2 if depth is not None else wo
    for what, x, n in (("rgb", rgb, B * h * w * 3), ("depth", depth, B * h * w)):
        if x is None:
            continue
        if x.dtype != torch.float32 or not x.is_contiguous() or x.device != out.device:
            raise ValueError(f"pack_frames: {what} must be a contiguous fp32 tensor on out's device")
        if x.numel() != n or (depth is not None and wo % 2):
            raise ValueError(f"pack_frames: {what} of shape {tuple(x.shape)} does not fill frames of {tuple(out.shape)}")
    with torch.cuda.device(out.device):
        table = _jet_on(out.device) if depth is not None else None
        _hip.call("cpn_pack_frames", rgb.data_ptr(), depth.data_ptr() if depth is not None else None,
                  table.data_ptr() if table is not None else None, B, h, w, out.data_ptr(), _hip.stream_handle())
    return out


@torch.no_grad()
def render_path(model, model_input: Dict, t, sway: float = 0.0, depth: bool = False,
                window: Optional[Sequence[int]] = None, return_rgb: bool = False, turns: float = 2.0,
                announce: bool = True, return_depth: bool = False) -> Dict[str, torch.Tensor]:
    """Views along camera_path(rel_pose, t, sway, turns) of the pair in model_input (prepare_pair's dict, or any dict
    forward(val=True) takes: with val=True the geometry uses the estimated pose, not the context poses).

    get_z runs once; every pose k is one `model(input_k, z=z, rel_pose=rel_pose, val=True, flow=flow)` whose input differs
    from model_input in `query.cam2world` = poses[k] (and in the query pixels, with `window`).  Pose k + 1 is announced with
    model.prepare_next before frame k is queued (announce=False leaves that out: the same frames, each frame's host pose
    algebra then waits behind the previous render).  cpn_pack_frames writes frame k straight into the output.

    window=(y0, x0, h, w) renders that rectangle of the pixel grid only (tiles); None the whole size x size image.
    Returns a dict of device tensors: `frames` (K, B, h, w, 3) uint8, or (K, B, h, 2 w, 3) with depth=True (the right half is
    the `jet` panel of depth_ray / 10); `poses` (K, B, 4, 4); `rel_pose` (B, 4, 4) as get_z estimated it; with
    return_rgb=True also `rgb` (K, B, h * w, 3) fp32 as forward returned it; with return_depth=True also `depth` (K, B, h * w)
    fp32, forward's `depth_ray`, and `valid` (K, B, h * w) uint8, 1 where forward's `valid_mask` is not zero (the ray meets
    at least one of the two views) - what coponerf_amd.point_cloud starts from.  Nothing is read on the host here; forward's
    own contractual copy of `pixel_val` to pinned host memory stays (asynchronous, on a stream of its own)."""
    ctx, qry = model_input["context"], model_input["query"]
    S = int(ctx["rgb"].shape[2])
    B = int(ctx["rgb"].shape[0])
    dev = ctx["rgb"].device
    if ctx["rgb"].shape[3] != S:
        raise ValueError(f"render_path: square context images, got {tuple(ctx['rgb'].shape)}")
    y0, x0, h, w = (0, 0, S, S) if window is None else (int(v) for v in window)
    if not (0 <= y0 and 0 <= x0 and h >= 1 and w >= 1 and y0 + h <= S and x0 + w <= S):
        raise ValueError(f"render_path: window {tuple(window)} does not lie in the {S} x {S} grid")
    z, rel_pose, flow = model.get_z(model_input)
    poses = camera_path(rel_pose, t, sway=sway, turns=turns)
    K = int(poses.shape[0])
    R = h * w
    grid = _uv_grid(S, dev).view(S, S, 2)[y0:y0 + h, x0:x0 + w].reshape(1, 1, R, 2)
    uv = grid.expand(B, 1, R, 2).contiguous()
    blank = torch.zeros(B, 1, R, 3, dtype=torch.float32, device=dev)
    # one input dict per pose, made before the loop: the engine matches what prepare_next built to the later forward by the
    # identity of the camera tensors
    inputs = [{"context": ctx, "query": {"uv": uv, "rgb": blank, "intrinsics": qry["intrinsics"], "cam2world": poses[k].unsqueeze(1)}}
              for k in range(K)]
    frames = torch.empty(K, B, h, 2 * w if depth else w, 3, dtype=torch.uint8, device=dev)
    rgbs = torch.empty(K, B, R, 3, dtype=torch.float32, device=dev) if return_rgb else None
    depths = torch.empty(K, B, R, dtype=torch.float32, device=dev) if return_depth else None
    valids = torch.empty(K, B, R, dtype=torch.uint8, device=dev) if return_depth else None
    for k in range(K):
        if announce and k + 1 < K:
            model.prepare_next(inputs[k + 1], z, rel_pose, flow)
        out = model(inputs[k], z=z, rel_pose=rel_pose, val=True, flow=flow)
        rgb = out["rgb"].contiguous()
        pack_frames(rgb, frames[k], out["depth_ray"].contiguous() if depth else None)
        if return_rgb:
            rgbs[k].copy_(rgb.view(B, R, 3))
        if return_depth:
            depths[k].copy_(out["depth_ray"].view(B, R))
            valids[k].copy_(out["valid_mask"].view(B, R) != 0)
    result = {"frames": frames, "poses": poses, "rel_pose": rel_pose}
    if return_rgb:
        result["rgb"] = rgbs
    if return_depth:
        result["depth"], result["valid"] = depths, valids
    return result
