"""The argument checks of point_cloud, matches, splat, mesh and raster, once.  A tensor that is not on the HIP device is a
RuntimeError, a wrong dtype, shape, layout or device a ValueError; every message names the entry point and the argument."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch

def device_tensors(who: str, named, dev: Optional[torch.device] = None, owner: str = "one device") -> torch.device:
    """`named` yields (what, tensor, dtype, shape or None): contiguous tensors on the HIP device `dev` (None: the first's) -> dev."""
    for what, x, dtype, shape in named:
        if not torch.is_tensor(x) or not x.is_cuda:
            raise RuntimeError(f"{who} runs on the HIP device only (coponerf_amd has no non-HIP compute path): {what}")
        dev = x.device if dev is None else dev
        if x.dtype != dtype or not x.is_contiguous() or x.device != dev or (shape is not None and tuple(x.shape) != shape):
            raise ValueError(f"{who}: {what} must be a contiguous {dtype} tensor{'' if shape is None else f' of shape {shape}'} on "
                             f"{owner}, got {tuple(x.shape)} {x.dtype}")
    return dev


def one_device(who: str, *tensors) -> None:
    """Contiguous tensors on the first one's HIP device, or a RuntimeError."""
    if not all(torch.is_tensor(x) and x.is_cuda and x.is_contiguous() and x.device == tensors[0].device for x in tensors):
        raise RuntimeError(f"{who}: contiguous tensors on one HIP device (coponerf_amd has no non-HIP compute path)")


def pair_intrinsics(who: str, intrinsics: torch.Tensor, B: int) -> torch.Tensor:
    """intrinsics (B, 4, 4), or `query.intrinsics` (B, 1, 4, 4) -> the contiguous (B, 4, 4) tensor."""
    if intrinsics.dim() == 4 and intrinsics.shape[1] == 1:
        intrinsics = intrinsics[:, 0]
    if tuple(intrinsics.shape) != (B, 4, 4):
        raise ValueError(f"{who}: intrinsics must be (B, 4, 4) or (B, 1, 4, 4) with B = {B}, got {tuple(intrinsics.shape)}")
    return intrinsics.contiguous()


def view_cameras(who: str, poses: torch.Tensor, intrinsics: torch.Tensor, B: int, cap: int, H: int, W: int, dev: torch.device,
                 owner: str, max_side: Optional[int] = None) -> Tuple[int, torch.Tensor]:
    """poses (K, B, 4, 4) and intrinsics on `dev`, H x W images (no side beyond max_side), `cap` rows to draw -> (K, intrinsics)."""
    if max_side is not None and (H > max_side or W > max_side):
        raise ValueError(f"{who}: need H, W <= {max_side}, got H = {H}, W = {W}")
    device_tensors(who, (("poses", poses, torch.float32, None), ("intrinsics", intrinsics, torch.float32, None)), dev, owner)
    if poses.dim() != 4 or int(poses.shape[1]) != B or poses.shape[2:] != (4, 4):
        raise ValueError(f"{who}: poses must be (K, B, 4, 4) with B = {B}, got {tuple(poses.shape)}")
    Kb = pair_intrinsics(who, intrinsics, B)
    K = int(poses.shape[0])
    if not 1 <= K <= 255 or H < 1 or W < 1 or K * B * H * W >= 2 ** 31 or cap < 1 or K * B * -(-cap // 256) >= 2 ** 31:
        raise ValueError(f"{who}: need 1 <= K <= 255 cameras, H, W, cap >= 1, K B H W < 2^31 and K B ceil(cap / 256) < 2^31, got "
                         f"K = {K}, B = {B}, H = {H}, W = {W}, cap = {cap}")
    return K, Kb


def zbuffer_dims(who: str, zbuf: torch.Tensor, B: int) -> Tuple[int, int, int, int]:
    """(K, B, H, W) of a z-buffer of int64 keys for B pairs, as splat_points and raster_faces return it."""
    if zbuf.dtype != torch.int64 or zbuf.dim() != 4 or int(zbuf.shape[1]) != B:
        raise ValueError(f"{who}: zbuf must be a (K, B, H, W) int64 tensor with B = {B}, got {tuple(zbuf.shape)} {zbuf.dtype}")
    return tuple(int(v) for v in zbuf.shape)


def background_word(who: str, background: Sequence[int]) -> int:
    """Three background bytes -> r | g << 8 | b << 16, the form the resolve kernels take."""
    bg = [int(v) for v in background]
    if len(bg) != 3 or not all(0 <= v <= 255 for v in bg):
        raise ValueError(f"{who}: background must be three bytes, got {tuple(background)}")
    return bg[0] | bg[1] << 8 | bg[2] << 16


def frame_outputs(K: int, B: int, H: int, W: int, dev: torch.device, depth: bool, index: bool,
                  bary: bool = False) -> Tuple[Dict[str, torch.Tensor], List[Optional[int]]]:
    """A resolve's dict of `frames` and, as asked for, `depth`, `index` and `bary`; and their four pointers, None where not asked."""
    kinds = (("frames", True, (3,), torch.uint8), ("depth", depth, (), torch.float32), ("index", index, (), torch.int32),
             ("bary", bary, (3,), torch.float32))
    out = {name: torch.empty((K, B, H, W) + tail, dtype=dtype, device=dev) for name, asked, tail, dtype in kinds if asked}
    return out, [out[name].data_ptr() if name in out else None for name, *_ in kinds]
