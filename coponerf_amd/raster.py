"""A Mesh's triangles drawn into any camera through a z-buffer: the fused surface made visible on a headless machine, closed
where it is closed and hiding what lies behind it, and a check of it against the two photos that needs no ground truth.

  raster_faces   the triangles into K cameras: a (K, B, H, W) z-buffer of (depth bits, face index) keys: cpn_raster_faces
  resolve        a z-buffer -> frames, depth, face index and weights: cpn_raster_resolve
  draw           the two together: the (K, B, H, W, 3) uint8 frames render_path and splat.draw return
  photo_check    the fused surface drawn into the two photos' own cameras and scored against them

splat.orbit_poses and novel_views.camera_path are the camera sources; splat.score scores a result unchanged (`index >= 0` means
covered).  There is no fill pass: a triangle surface has no holes between samples.

**No clipping (a face with a vertex nearer than `near` is not drawn at all), the snap of the projected vertices to 1/256 pixel, the
top-left fill rule, the tie rule (equal fp32 depths fall to the lower face index), the headlight and photo_check are this
package's definitions (include/coponerf_hip.h), not the reference's, which has no rasteriser.  None of it has been tried on a
trained checkpoint, because none is available offline.**  Left out: clipping against the near plane, antialiasing and
blending, texture maps, smooth (per-vertex) normals, wireframe, video encoding, a differentiable rasteriser.
"""
from __future__ import annotations

from typing import Dict, Sequence, Tuple

import torch

from . import _hip
from ._args import background_word, device_tensors, frame_outputs, view_cameras, zbuffer_dims
from .novel_views import render_path
from .splat import score_photo

SHADES = {"colour": 0, "headlight": 1}
MAX_SIDE = 16384


def _mesh(who: str, mesh) -> Tuple[int, int, int]:
    xyz = mesh.xyz
    device_tensors(who, (("mesh.xyz", mesh.xyz, torch.float32, None), ("mesh.rgb", mesh.rgb, torch.uint8, None),
                         ("mesh.nvert", mesh.nvert, torch.int32, None), ("mesh.faces", mesh.faces, torch.int32, None),
                         ("mesh.nface", mesh.nface, torch.int32, None)), owner="the mesh's device")
    B = int(xyz.shape[0]) if xyz.dim() == 3 else -1
    if xyz.dim() != 3 or xyz.shape[2] != 3 or mesh.rgb.shape != xyz.shape or mesh.faces.dim() != 3 or \
            tuple(mesh.faces.shape[::2]) != (B, 3) or tuple(mesh.nvert.shape) != (B,) or tuple(mesh.nface.shape) != (B,):
        raise ValueError(f"{who}: a Mesh of xyz and rgb (B, max_vertices, 3), faces (B, max_faces, 3), nvert and nface (B), got "
                         f"{tuple(xyz.shape)}, {tuple(mesh.rgb.shape)}, {tuple(mesh.faces.shape)}, {tuple(mesh.nvert.shape)} and "
                         f"{tuple(mesh.nface.shape)}")
    capv, capf = int(xyz.shape[1]), int(mesh.faces.shape[1])
    if capv < 1 or capf < 1:
        raise ValueError(f"{who}: the mesh needs room for at least one vertex and one face, got {capv} and {capf}")
    return B, capv, capf


@torch.no_grad()
def raster_faces(mesh, poses: torch.Tensor, intrinsics: torch.Tensor, H: int, W: int, cull: bool = False,
                 near: float = 1e-3) -> torch.Tensor:
    """cpn_raster_faces: the z-buffer (K, B, H, W) of the mesh's triangles in the cameras `poses` (K, B, 4, 4) fp32, camera to
    reference (camera_path's, orbit_poses'), with `intrinsics` (B, 4, 4) or (B, 1, 4, 4) fp32 of the H x W output image.  An
    int64 tensor holding uint64 keys: (bits of the fp32 depth) << 32 | face row, -1 (all ones) where no face fell.  cull=True
    drops the faces seen from behind (the front is the side Volume.extract winds towards, the cameras' free space).  No
    clipping: a face with a vertex nearer than `near` is not drawn at all."""
    H, W = int(H), int(W)
    B, capv, capf = _mesh("raster_faces", mesh)
    K, Kb = view_cameras("raster_faces", poses, intrinsics, B, capf, H, W, mesh.xyz.device, "the mesh's device", MAX_SIDE)
    if not float(near) > 0.0:
        raise ValueError(f"raster_faces: need near > 0, got {near}")
    zbuf = torch.empty(K, B, H, W, dtype=torch.int64, device=mesh.xyz.device)
    with torch.cuda.device(zbuf.device):
        _hip.call("cpn_raster_faces", mesh.xyz.data_ptr(), mesh.nvert.data_ptr(), mesh.faces.data_ptr(), mesh.nface.data_ptr(),
                  poses.data_ptr(), Kb.data_ptr(), K, B, capv, capf, H, W, 1 if cull else 0, float(near), zbuf.data_ptr(),
                  _hip.stream_handle())
    return zbuf


@torch.no_grad()
def resolve(zbuf: torch.Tensor, mesh, poses: torch.Tensor, intrinsics: torch.Tensor, shade: str = "colour",
            background: Sequence[int] = (0, 0, 0), return_depth: bool = False, return_index: bool = False,
            return_bary: bool = False) -> Dict[str, torch.Tensor]:
    """cpn_raster_resolve: raster_faces' z-buffer (K, B, H, W), with the mesh and the cameras it was drawn with -> `frames`
    (K, B, H, W, 3) uint8; on request `depth` (K, B, H, W) fp32 (the z-depth in the camera, NaN where empty), `index`
    (K, B, H, W) int32 (the row of mesh.faces, -1 where empty) and `bary` (K, B, H, W, 3) fp32 (the perspective-correct weights
    of the face's three vertices, NaN where empty).  shade="colour": the vertices' bytes, interpolated perspective-correctly;
    shade="headlight": a grey |n . d| of the face normal and the pixel's ray, which shows a surface's shape where the vertex
    colours say nothing.  background: the empty pixels' bytes.  There is no fill pass: a triangle surface has no holes
    between samples."""
    B, capv, capf = _mesh("resolve", mesh)
    dev = device_tensors("resolve", (("zbuf", zbuf, torch.int64, None),), mesh.xyz.device, "the mesh's device")
    nk, _, H, W = zbuffer_dims("resolve", zbuf, B)
    K, Kb = view_cameras("resolve", poses, intrinsics, B, capf, H, W, dev, "the mesh's device", MAX_SIDE)
    if K != nk:
        raise ValueError(f"resolve: zbuf holds {nk} cameras, poses {K}")
    if shade not in SHADES:
        raise ValueError(f"resolve: need shade in {tuple(SHADES)}, got {shade!r}")
    word = background_word("resolve", background)
    out, (frames, depth, index, bary) = frame_outputs(K, B, H, W, dev, return_depth, return_index, return_bary)
    with torch.cuda.device(dev):
        _hip.call("cpn_raster_resolve", zbuf.data_ptr(), mesh.xyz.data_ptr(), mesh.rgb.data_ptr(), mesh.nvert.data_ptr(),
                  mesh.faces.data_ptr(), poses.data_ptr(), Kb.data_ptr(), K, B, capv, capf, H, W, SHADES[shade], word, frames, depth,
                  index, bary, _hip.stream_handle())
    return out


@torch.no_grad()
def draw(mesh, poses: torch.Tensor, intrinsics: torch.Tensor, H: int, W: int, cull: bool = False, near: float = 1e-3,
         shade: str = "colour", background: Sequence[int] = (0, 0, 0), return_depth: bool = False, return_index: bool = False,
         return_bary: bool = False) -> Dict[str, torch.Tensor]:
    """The mesh as the K cameras `poses` see it: raster_faces, then resolve.  The nearest face wins a pixel, the lower row of
    mesh.faces among equal depths.  Returns resolve's dict of device tensors: `frames` (K, B, H, W, 3) uint8 as render_path's
    and splat.draw's, and what was asked for of `depth`, `index` and `bary`.  Two launches and a memset; nothing is read on
    the host."""
    zbuf = raster_faces(mesh, poses, intrinsics, H, W, cull=cull, near=near)
    return resolve(zbuf, mesh, poses, intrinsics, shade=shade, background=background, return_depth=return_depth,
                   return_index=return_index, return_bary=return_bary)


@torch.no_grad()
def photo_check(model, model_input: Dict, t=(0.0, 0.25, 0.5, 0.75, 1.0), cull: bool = False,
                **reconstruct_kwargs) -> Tuple[torch.Tensor, torch.Tensor]:
    """Does the fused surface land on the two photos?  (coverage (2, B), psnr (2, B)) float64 on the device, needing nothing
    but the pair.

    render_path renders the views t once (t[0] == 0 and t[-1] == 1: the two photos' own cameras are among them), with depth;
    mesh.integrate fuses them and Volume.extract takes the surface (reconstruct_kwargs: dims, bounds, trunc_voxels, window of
    integrate; min_weight, max_vertices, max_faces of extract).  Row 0: the surface drawn into view 0's camera (render_path's
    `poses[0]`) with photo 0's own context intrinsics and scored against photo 0 (`context.rgb[:, 0]` as bytes, pack_frames) by
    splat.score; row 1: into view 1's ESTIMATED camera (`poses[-1]`) with photo 1's intrinsics, against photo 1.  Unlike
    splat.cross_view_check the surface occludes, and it is the fusion of every view: a high coverage with a low PSNR says
    that the surface lands in the photo but carries the wrong colours; a low coverage that integrate's box or truncation, or
    extract's min_weight, left little of it.  This package's definition; not tried on a trained checkpoint."""
    from .mesh import integrate
    t = tuple(float(v) for v in t)
    if len(t) < 2 or t[0] != 0.0 or t[-1] != 1.0:
        raise ValueError(f"photo_check: t must start at 0 and end at 1 (the two photos' own cameras), got {t}")
    fuse = {k: reconstruct_kwargs.pop(k) for k in ("dims", "bounds", "trunc_voxels", "window") if k in reconstruct_kwargs}
    take = {k: reconstruct_kwargs.pop(k) for k in ("min_weight", "max_vertices", "max_faces") if k in reconstruct_kwargs}
    if reconstruct_kwargs:
        raise TypeError(f"photo_check: unknown arguments {sorted(reconstruct_kwargs)}")
    ctx = model_input["context"]
    S = int(ctx["rgb"].shape[2])
    res = render_path(model, model_input, t, window=fuse.get("window"), return_rgb=True, return_depth=True)
    surface = integrate(res, model_input["query"]["intrinsics"], S, **fuse).extract(**take)
    scores = []
    for view, k in ((0, 0), (1, len(t) - 1)):
        out = draw(surface, res["poses"][k:k + 1].contiguous(), ctx["intrinsics"][:, view].contiguous(), S, S, cull=cull,
                   return_index=True)
        scores.append(score_photo(out, ctx["rgb"][:, view]))
    return torch.stack([c for c, _ in scores]), torch.stack([p for _, p in scores])
