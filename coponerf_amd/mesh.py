"""Two photos in, a coloured triangle mesh out: the rendered depth maps fused in a voxel volume, and its zero level set.

`depth_ray` is the depth of ONE of 2 x 64 samples, so every rendered depth map is a staircase (point_cloud.py).  A truncated
signed distance averaged per voxel over the K views of render_path places the surface between the steps; naive surface nets
(one vertex per cell that the surface crosses, one quad per lattice edge that it crosses: no triangle table) turns it into a mesh.

  bounds        the box of the valid points of point_cloud.unproject, per pair, on the device
  integrate     the K views of render_path -> a Volume: cpn_tsdf_integrate
  Volume        tsdf / weight / colour on the device; extract() -> a Mesh: cpn_surface_vertices, cpn_surface_faces
  Mesh          xyz / rgb / nvert / faces / nface on the device; numpy(b) is the one host read, ply_bytes / save write a binary
                PLY, cloud() hands the vertices to splat.draw as a PointCloud, frames() the triangles to raster.draw
  reconstruct   novel_views.render_path, integrate, extract

**The TSDF rule (the projective distance along z, the nearest pixel, uniform weights, the colour averaged over every updating
view), the surface-nets vertex rule, the observed-cell rule and the defaults of `dims`, `trunc_voxels` and the box are this
package's definitions (include/coponerf_hip.h), not the reference's, which has no mesh.  None of it has been tried on a trained
checkpoint, because none is available offline.**  Surface nets can produce non-manifold edges in ambiguous cells.  The box of
`bounds` is the raw extent of the valid points, so outliers stretch it: pass your own.  Left out: marching cubes, normals,
decimation and smoothing, texture maps, weighting by view angle (coponerf_amd.raster draws the triangles: Mesh.frames).  Writing
the PLY is the only file I/O.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _hip
from ._args import device_tensors
from .novel_views import render_path
from .point_cloud import PointCloud, _views, ply_vertices, unproject

MAX_VERTICES = 2 ** 22                                        # the default capacity of extract never exceeds it


def _dims(who: str, dims: Sequence[int], B: int) -> Tuple[int, int, int]:
    if len(dims) != 3:
        raise ValueError(f"{who}: dims must be (Nx, Ny, Nz), got {tuple(dims)}")
    Nx, Ny, Nz = (int(v) for v in dims)
    if min(Nx, Ny, Nz) < 2 or B * Nx * Ny * Nz >= 2 ** 31:
        raise ValueError(f"{who}: need Nx, Ny, Nz >= 2 and B Nx Ny Nz < 2^31, got B = {B}, dims = {(Nx, Ny, Nz)}")
    return Nx, Ny, Nz


@torch.no_grad()
def bounds(views: Dict[str, torch.Tensor], intrinsics: torch.Tensor, S: int,
           window: Optional[Sequence[int]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(lo, hi), each (B, 3) fp32 on the device: the per-axis minimum and maximum of the valid points of
    point_cloud.unproject(views["depth"], views["poses"], ...) over all K views, in stock ops; nothing is read on the host.  A
    pair without a valid point gives NaN, which integrate turns into the empty volume.  The raw extent: one outlier stretches it."""
    xyz = unproject(views["depth"], views["poses"], intrinsics, S, window=window)            # (K, B, h w, 3), NaN where invalid
    B = int(xyz.shape[1])
    pts = xyz.permute(1, 0, 2, 3).reshape(B, -1, 3)
    bad = torch.isnan(pts)
    lo = torch.where(bad, float("inf"), pts).amin(dim=1)
    hi = torch.where(bad, float("-inf"), pts).amax(dim=1)
    none = bad.all(dim=1)
    return torch.where(none, float("nan"), lo), torch.where(none, float("nan"), hi)


_bounds = bounds                                              # integrate's argument of the same name hides the function


@torch.no_grad()
def integrate(views: Dict[str, torch.Tensor], intrinsics: torch.Tensor, S: int, dims: Sequence[int] = (128, 128, 128),
              bounds: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, trunc_voxels: float = 3.0,
              window: Optional[Sequence[int]] = None) -> "Volume":
    """cpn_tsdf_integrate: `views`, the dict render_path(..., return_rgb=True, return_depth=True) returned for `window` (`depth`
    (K, B, h * w) fp32, `valid` (K, B, h * w) uint8, `rgb` (K, B, h * w, 3) fp32, `poses` (K, B, 4, 4) fp32), as
    point_cloud.from_views takes it -> the Volume of dims = (Nx, Ny, Nz) voxels per pair over the box bounds = (lo, hi), each
    (B, 3) fp32 on the device in view 0's frame (None: bounds(views, ...)).  spacing = (hi - lo) / (N - 1) per axis and
    trunc = trunc_voxels * max(spacing), both formed on the device; a pair whose box is NaN or flat along an axis gets the empty
    volume.  One launch; nothing is read on the host."""
    depth, valid, rgb, poses = views["depth"], views["valid"], views["rgb"], views["poses"]
    K, B, y0, x0, h, w, Kb = _views("integrate", depth, poses, intrinsics, S, window)
    device_tensors("integrate", (("valid", valid, torch.uint8, (K, B, h * w)), ("rgb", rgb, torch.float32, (K, B, h * w, 3))),
                   depth.device, "depth's device")
    Nx, Ny, Nz = _dims("integrate", dims, B)
    if not float(trunc_voxels) > 0.0:
        raise ValueError(f"integrate: trunc_voxels must be > 0, got {trunc_voxels}")
    dev = depth.device
    lo, hi = _bounds(views, intrinsics, S, window=window) if bounds is None else bounds
    for what, x in (("lo", lo), ("hi", hi)):
        if not torch.is_tensor(x) or x.device != dev or x.dtype != torch.float32 or tuple(x.shape) != (B, 3):
            raise ValueError(f"integrate: bounds = (lo, hi), each a ({B}, 3) fp32 tensor on depth's device: {what}")
    # a tensor as the divisor: by a Python number torch multiplies with the rounded reciprocal on the device
    steps = torch.stack([torch.full((B,), float(n - 1), dtype=torch.float32, device=dev) for n in (Nx, Ny, Nz)], dim=1)
    origin = lo.contiguous()
    spacing = ((hi - lo) / steps).contiguous()
    trunc = (spacing.amax(dim=1) * float(trunc_voxels)).contiguous()
    tsdf = torch.empty(B, Nz, Ny, Nx, dtype=torch.float32, device=dev)
    weight = torch.empty(B, Nz, Ny, Nx, dtype=torch.uint8, device=dev)
    colour = torch.empty(B, Nz, Ny, Nx, 3, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _hip.call("cpn_tsdf_integrate", depth.data_ptr(), valid.data_ptr(), rgb.data_ptr(), poses.data_ptr(), Kb.data_ptr(),
                  origin.data_ptr(), spacing.data_ptr(), trunc.data_ptr(), K, B, int(S), y0, x0, h, w, Nx, Ny, Nz, tsdf.data_ptr(),
                  weight.data_ptr(), colour.data_ptr(), _hip.stream_handle())
    return Volume(tsdf, weight, colour, origin, spacing, trunc, (Nx, Ny, Nz))


class Volume:
    """The fused volumes of B pairs on the device: tsdf (B, Nz, Ny, Nx) fp32 (the mean truncated signed distance in units of
    trunc, negative behind the surface, 1 where no view updated), weight (B, Nz, Ny, Nx) uint8 (the number of updating views),
    colour (B, Nz, Ny, Nx, 3) fp32 in [-1, 1], origin (B, 3), spacing (B, 3) and trunc (B) fp32, dims = (Nx, Ny, Nz).  Voxel
    (ix, iy, iz) of pair b sits at origin[b] + (ix, iy, iz) * spacing[b] in view 0's frame."""

    def __init__(self, tsdf: torch.Tensor, weight: torch.Tensor, colour: torch.Tensor, origin: torch.Tensor,
                 spacing: torch.Tensor, trunc: torch.Tensor, dims: Sequence[int]):
        self.tsdf, self.weight, self.colour = tsdf, weight, colour
        self.origin, self.spacing, self.trunc = origin, spacing, trunc
        self.dims = tuple(int(v) for v in dims)

    @torch.no_grad()
    def extract(self, min_weight: int = 1, max_vertices: Optional[int] = None, max_faces: Optional[int] = None) -> "Mesh":
        """Naive surface nets: cpn_surface_vertices, then cpn_surface_faces; four launches, nothing is read on the host.  A cell
        carries a vertex iff all eight of its corners were updated by at least min_weight views and the sign of tsdf changes
        among them.  max_vertices and max_faces are CAPACITIES, not estimates: the rows the Mesh has room for (default
        min(cells, 2^22) and 3 * max_vertices).  The counts it reports are the true ones; Mesh.numpy raises where they exceed
        the capacity."""
        Nx, Ny, Nz = self.dims
        B = int(self.tsdf.shape[0])
        dev = self.tsdf.device
        want = (("tsdf", self.tsdf, torch.float32, (B, Nz, Ny, Nx)), ("weight", self.weight, torch.uint8, (B, Nz, Ny, Nx)),
                ("colour", self.colour, torch.float32, (B, Nz, Ny, Nx, 3)), ("origin", self.origin, torch.float32, (B, 3)),
                ("spacing", self.spacing, torch.float32, (B, 3)))
        device_tensors("extract", want, dev, "the volume's device")
        lib = _hip.lib()
        n_vert, n_face = lib.cpn_surface_vertices_scratch(B, Nx, Ny, Nz), lib.cpn_surface_faces_scratch(B, Nx, Ny, Nz)
        if n_vert <= 0 or n_face <= 0:
            raise ValueError(f"extract: need 1 <= B <= 65535, dims >= 2 and 3 B Nx Ny Nz < 2^31, got B = {B}, dims = {self.dims}")
        if not 1 <= int(min_weight) <= 255:
            raise ValueError(f"extract: min_weight must lie in [1, 255], got {min_weight}")
        cells = (Nx - 1) * (Ny - 1) * (Nz - 1)
        capv = min(cells, MAX_VERTICES) if max_vertices is None else int(max_vertices)
        capf = 3 * capv if max_faces is None else int(max_faces)
        if capv < 1 or capf < 1 or B * capv >= 2 ** 31 or B * capf >= 2 ** 31:
            raise ValueError(f"extract: need 1 <= max_vertices, max_faces and B times either < 2^31, got {capv} and {capf}")
        xyz = torch.empty(B, capv, 3, dtype=torch.float32, device=dev)
        rgb = torch.empty(B, capv, 3, dtype=torch.uint8, device=dev)
        nvert = torch.empty(B, dtype=torch.int32, device=dev)
        cell_vertex = torch.empty(B, cells, dtype=torch.int32, device=dev)
        faces = torch.empty(B, capf, 3, dtype=torch.int32, device=dev)
        nface = torch.empty(B, dtype=torch.int32, device=dev)
        scratch = torch.empty(max(n_vert, n_face), dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _hip.call("cpn_surface_vertices", self.tsdf.data_ptr(), self.weight.data_ptr(), self.colour.data_ptr(),
                      self.origin.data_ptr(), self.spacing.data_ptr(), B, Nx, Ny, Nz, int(min_weight), capv, scratch.data_ptr(),
                      xyz.data_ptr(), rgb.data_ptr(), nvert.data_ptr(), cell_vertex.data_ptr(), _hip.stream_handle())
            _hip.call("cpn_surface_faces", self.tsdf.data_ptr(), cell_vertex.data_ptr(), B, Nx, Ny, Nz, capf, scratch.data_ptr(),
                      faces.data_ptr(), nface.data_ptr(), _hip.stream_handle())
        return Mesh(xyz, rgb, nvert, faces, nface)


class Mesh:
    """The meshes of B pairs on the device: xyz (B, max_vertices, 3) fp32 in view 0's frame, rgb (B, max_vertices, 3) uint8, nvert
    (B) int32, faces (B, max_faces, 3) int32 (rows of xyz, the normals towards the cameras' free space) and nface (B) int32.
    Pair b's vertices are the rows [0, nvert[b]) in (cz, cy, cx) order of their cells, its triangles the rows [0, nface[b]); the
    rows beyond are not written.  The counts are the true ones even where they exceed the capacities."""

    def __init__(self, xyz: torch.Tensor, rgb: torch.Tensor, nvert: torch.Tensor, faces: torch.Tensor, nface: torch.Tensor):
        self.xyz, self.rgb, self.nvert, self.faces, self.nface = xyz, rgb, nvert, faces, nface

    @torch.no_grad()
    def numpy(self, b: int = 0) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Pair b's mesh on the host: ((n, 3) float32, (n, 3) uint8, (m, 3) int32).  ONE read: the two counts, the positions,
        the colours and the triangles of the pair travel in one buffer of the capacities' size (a lower max_vertices makes a
        smaller read), the rows beyond the counts are dropped on the host.  Raises if a count exceeds its capacity."""
        capv, capf = int(self.xyz.shape[1]), int(self.faces.shape[1])
        packed = torch.cat((self.nvert[b:b + 1].view(torch.uint8), self.nface[b:b + 1].view(torch.uint8),
                            self.xyz[b].view(torch.uint8).reshape(-1), self.faces[b].view(torch.uint8).reshape(-1),
                            self.rgb[b].reshape(-1))).cpu().numpy()
        n, m = (int(v) for v in packed[:8].view(np.int32))
        if n > capv or m > capf:
            raise RuntimeError(f"Mesh.numpy: pair {b} has {n} vertices and {m} triangles, the capacities are max_vertices = {capv} "
                               f"and max_faces = {capf}: extract again with room for them")
        xyz = packed[8:8 + 12 * capv].view(np.float32).reshape(capv, 3)[:n].copy()
        faces = packed[8 + 12 * capv:8 + 12 * capv + 12 * capf].view(np.int32).reshape(capf, 3)[:m].copy()
        rgb = packed[8 + 12 * capv + 12 * capf:].reshape(capv, 3)[:n].copy()
        return xyz, rgb, faces

    def ply_bytes(self, b: int = 0) -> bytes:
        """Pair b as a binary little-endian PLY: point_cloud.ply_bytes' vertices and `list uchar int vertex_indices` faces."""
        return ply_bytes(*self.numpy(b))

    def save(self, path, b: int = 0) -> None:
        with open(path, "wb") as f:
            f.write(self.ply_bytes(b))

    def cloud(self) -> PointCloud:
        """The vertices as a PointCloud (the count clamped to the capacity, on the device): splat.draw(mesh.cloud(), ...)
        previews the mesh's vertices alone; frames() draws its triangles."""
        return PointCloud(self.xyz, self.rgb, torch.clamp(self.nvert, max=int(self.xyz.shape[1])))

    def frames(self, poses: torch.Tensor, intrinsics: torch.Tensor, H: int, W: int, **kwargs) -> Dict[str, torch.Tensor]:
        """The mesh's triangles as the cameras `poses` (K, B, 4, 4) see them, on the device: coponerf_amd.raster.draw(self, ...)."""
        from .raster import draw
        return draw(self, poses, intrinsics, H, W, **kwargs)


def ply_bytes(xyz: np.ndarray, rgb: np.ndarray, faces: np.ndarray) -> bytes:
    """A binary little-endian PLY of n vertices (xyz (n, 3) float32, rgb (n, 3) uint8: point_cloud.ply_bytes' vertex element) and m
    triangles (faces (m, 3) int32); the header is built here, on the host."""
    faces = np.asarray(faces)
    m = int(faces.shape[0])
    if faces.shape != (m, 3) or faces.dtype != np.int32:
        raise ValueError(f"ply_bytes: faces (m, 3) int32, got {faces.shape} {faces.dtype}")
    header, rows = ply_vertices(xyz, rgb)
    tris = np.empty(m, dtype=np.dtype([("n", "u1"), ("v", "<i4", 3)]))
    tris["n"], tris["v"] = 3, faces
    return (header + f"element face {m}\nproperty list uchar int vertex_indices\nend_header\n").encode("ascii") + rows + tris.tobytes()


@torch.no_grad()
def reconstruct(model, model_input: Dict, t=(0.0, 0.25, 0.5, 0.75, 1.0), dims: Sequence[int] = (128, 128, 128),
                bounds: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, trunc_voxels: float = 3.0, min_weight: int = 1,
                window: Optional[Sequence[int]] = None, max_vertices: Optional[int] = None,
                max_faces: Optional[int] = None) -> Mesh:
    """The mesh of the pair(s) in model_input (prepare_pair's dict), in view 0's frame: render_path renders the K = len(t) views
    along the estimated camera path with their depth, integrate fuses them, Volume.extract takes the surface.  Nothing is read on
    the host here beyond what render_path documents (forward's own `pixel_val` copy); Mesh.numpy is the read."""
    S = int(model_input["context"]["rgb"].shape[2])
    res = render_path(model, model_input, t, window=window, return_rgb=True, return_depth=True)
    volume = integrate(res, model_input["query"]["intrinsics"], S, dims=dims, bounds=bounds, trunc_voxels=trunc_voxels, window=window)
    return volume.extract(min_weight=min_weight, max_vertices=max_vertices, max_faces=max_faces)
