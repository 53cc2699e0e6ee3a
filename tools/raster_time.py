"""What coponerf_amd.raster costs (csrc/raster.hip), on one MI355X, by HIP events: tools/mesh_time.py's workload -
five analytic 256 x 256 views of a sphere in front of a wall fused at 128^3 and at 256^3 - drawn into 60 orbit cameras at 256 x 256.

  (a) cpn_raster_faces and cpn_raster_resolve alone, into buffers made once, and raster.draw as a user calls it: per call of 60
      frames and per frame.  Beside them, in the same run: splat.draw of Mesh.cloud() into the same cameras, and the
      integrate + extract that made the mesh.  The launch covers the mesh's CAPACITY (extract's default: 3 x min(cells, 2^22) rows
      of faces), so the same draw is also timed on a mesh extracted with room for just its faces.
  (b) the cost of large faces: the same 60 cameras at a third of the distance from the pivot, where faces cover hundreds of
      pixels, and two triangles that fill a 1024 x 1024 image, alone.  Run the script a second time with COPONERF_HIP_LIB naming a
      build whose CPN_RASTER_SMALL is so large that every face takes the one-lane walk (--large-only): the ratio of the two is
      what the wave's walk earns.
  (c) with --model: one render_path frame of the synthetic-weight model, for scale.

    python tools/raster_time.py [--rounds 5] [--iters 50] [--model] [--large-only] [--out profiles/r19_raster.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mesh_time import HI, LO, S, analytic_views, measure                              # noqa: E402
from coponerf_amd import _hip, mesh, raster, splat, synthetic as syn                  # noqa: E402

CAMERAS, PIVOT_Z, YAW = 60, 3.0, 40.0


def orbit(dev, scale=1.0):
    """splat.orbit_poses' 60 cameras, or the same cameras at `scale` times their distance from the pivot."""
    M = splat.orbit_matrices(CAMERAS, PIVOT_Z, YAW, 5.0)
    pivot = np.array([0.0, 0.0, PIVOT_Z])
    for k in range(CAMERAS):
        M[k, :3, 3] = pivot - scale * (M[k, :3, :3] @ pivot)
    return torch.from_numpy(M.astype(np.float32)).unsqueeze(1).contiguous().to(dev)


def covered_pixels_per_face(m, poses, intr, H, W):
    """(drawn faces that win a pixel, covered pixels) of camera 0: what 'large' means in numbers."""
    index = raster.draw(m, poses[:1].contiguous(), intr, H, W, return_index=True)["index"]
    hit = index[index >= 0]
    return int(torch.unique(hit).numel()), int(hit.numel())


def draw_forms(m, poses, intr, H, W, tag):
    K = int(poses.shape[0])
    zbuf = raster.raster_faces(m, poses, intr, H, W)
    out = raster.resolve(zbuf, m, poses, intr)
    capv, capf = int(m.xyz.shape[1]), int(m.faces.shape[1])
    st = _hip.stream_handle()

    def faces():
        _hip.call("cpn_raster_faces", m.xyz.data_ptr(), m.nvert.data_ptr(), m.faces.data_ptr(), m.nface.data_ptr(), poses.data_ptr(),
                  intr.data_ptr(), K, 1, capv, capf, H, W, 0, 1e-3, zbuf.data_ptr(), st)

    def resolve():
        _hip.call("cpn_raster_resolve", zbuf.data_ptr(), m.xyz.data_ptr(), m.rgb.data_ptr(), m.nvert.data_ptr(), m.faces.data_ptr(),
                  poses.data_ptr(), intr.data_ptr(), K, 1, capv, capf, H, W, 0, 0, out["frames"].data_ptr(), None, None, None, st)

    return {f"{tag}: cpn_raster_faces": faces, f"{tag}: cpn_raster_resolve": resolve,
            f"{tag}: raster.draw": lambda: raster.draw(m, poses, intr, H, W)}


def two_triangles(dev, side=1024):
    """A quad at depth 2 that reaches beyond the side x side image of the identity camera, as two triangles."""
    f = float(side)
    intr = torch.tensor([[[f, 0, 0.5 * f, 0], [0, f, 0.5 * f, 0], [0, 0, 1, 0], [0, 0, 0, 1]]], dtype=torch.float32, device=dev)
    xyz = torch.tensor([[[-1.1, -1.1, 2.0], [1.1, -1.1, 2.0], [1.1, 1.1, 2.1], [-1.1, 1.1, 2.1]]], dtype=torch.float32, device=dev)
    m = mesh.Mesh(xyz, torch.full((1, 4, 3), 128, dtype=torch.uint8, device=dev), torch.tensor([4], dtype=torch.int32, device=dev),
                  torch.tensor([[[0, 1, 2], [0, 2, 3]]], dtype=torch.int32, device=dev), torch.tensor([2], dtype=torch.int32, device=dev))
    return m, torch.eye(4, device=dev).reshape(1, 1, 4, 4).contiguous(), intr


def per_frame(ms, frames):
    return {k: round(v / frames, 5) for k, v in ms.items() if k in ("median", "min", "max")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--model", action="store_true")
    ap.add_argument("--model-iters", type=int, default=3)
    ap.add_argument("--large-only", action="store_true", help="only the large-face workloads of (b), on the 128^3 mesh")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "raster_time.py measures on a HIP device"
    dev = torch.device("cuda:0")
    views, intr = analytic_views(dev)
    far, near = orbit(dev), orbit(dev, 1.0 / 3.0)
    lo, hi = torch.tensor([LO], device=dev), torch.tensor([HI], device=dev)
    res = {"device": torch.cuda.get_device_name(0), "library": os.path.basename(_hip.LIB_PATH), "RASTER_SMALL_of_the_header": _hip.CONSTANTS["RASTER_SMALL"],
           "workload": f"5 analytic views of {S} x {S} fused at N^3, drawn into {CAMERAS} orbit cameras at {S} x {S}; one pair",
           "iters": a.iters, "rounds": a.rounds, "unit": "ms per call of 60 frames (1 frame for the two triangles), HIP events, "
           "median / min / max of the rounds; per_frame_ms = that / 60", "meshes": {}}
    for N in (128,) if a.large_only else (128, 256):
        def fuse(**room):
            return mesh.integrate(views, intr, S, dims=(N, N, N), bounds=(lo, hi)).extract(**room)

        m = fuse()
        nvert, nface = int(m.nvert[0]), int(m.nface[0])
        tight = fuse(max_vertices=nvert, max_faces=nface)
        forms = {}
        if not a.large_only:
            forms.update(draw_forms(m, far, intr, S, S, "orbit"))
            forms.update({"orbit, capacity = the counts: " + k.split(": ")[1]: v for k, v in draw_forms(tight, far, intr, S, S, "t").items()})
            cloud = m.cloud()
            forms["orbit: splat.draw of Mesh.cloud()"] = lambda cloud=cloud: splat.draw(cloud, far, intr, S, S)
            forms["integrate + extract (box given)"] = fuse
        forms.update(draw_forms(tight, near, intr, S, S, "a third of the distance, capacity = the counts"))
        ms = measure(forms, a.rounds, a.iters)
        entry = {"vertices": nvert, "triangles": nface, "max_vertices": int(m.xyz.shape[1]), "max_faces": int(m.faces.shape[1]),
                 "orbit_camera_0 (faces that win a pixel, covered pixels)": covered_pixels_per_face(tight, far, intr, S, S),
                 "near_camera_0 (faces that win a pixel, covered pixels)": covered_pixels_per_face(tight, near, intr, S, S),
                 "ms": ms, "per_frame_ms": {k: per_frame(v, CAMERAS) for k, v in ms.items() if "integrate" not in k}}
        res["meshes"][f"{N}^3"] = entry
        del forms, m, tight
        torch.cuda.empty_cache()
    tri, eye, intr_big = two_triangles(dev)
    res["two triangles that fill 1024 x 1024, one camera"] = {"ms": measure(draw_forms(tri, eye, intr_big, 1024, 1024, "two triangles"),
                                                                              a.rounds, a.iters)}
    if a.model:
        from coponerf_amd import CoPoNeRF
        from coponerf_amd.novel_views import prepare_pair, render_path
        model = CoPoNeRF.CoPoNeRF(n_view=2)
        shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
        model.load_state_dict(syn.make_full_weights(shapes), strict=True)
        model = model.to(dev).eval()
        frames = syn.make_scene(n=2)[0]
        inp = prepare_pair(frames[0], frames[1], hfov_deg=75.0, device=dev)
        t = (0.0, 0.25, 0.5, 0.75, 1.0)
        ms = measure({"render_path_5_views (get_z + 5 forward)": lambda: render_path(model, inp, t, return_rgb=True, return_depth=True)},
                     a.rounds, a.model_iters)
        res["model"] = {"iters": a.model_iters, "ms": ms,
                        "per_frame_ms": {k: per_frame(v, len(t)) for k, v in ms.items()}}
    res["note"] = ("the launch of cpn_raster_faces covers the capacity of the mesh, not its count (nothing is read on the host to size a "
                   "grid), so the default capacities of extract cost threads that leave at once: 'capacity = the counts' is the same draw "
                   "on a mesh extracted with room for just its faces; the model carries synthetic weights (no trained checkpoint is "
                   "available); the analytic mesh is what TSDF fusion gives at these sizes, a user's own mesh may have larger faces")
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
