"""What coponerf_amd.mesh costs (csrc/mesh.hip), on one MI355X: five analytic 256 x 256 views of a sphere in front
of a wall (float64 ray casting on the host, rounded to fp32 once) fused into a 128^3 and a 256^3 volume, by HIP events.

  (a) cpn_tsdf_integrate alone, into buffers made once, against a stock-op composition of the same rule in float64 (projection
      by element-wise ops, a nearest gather, masked means), alternating in one process; the script says how far the two agree.
  (b) the two extraction stages alone, cpn_surface_vertices and cpn_surface_faces.  Extraction has no stock-op form without a
      host read (the number of vertices decides every later shape), so none is timed.
  (c) mesh.integrate + Volume.extract as a user calls them, with the box given and with bounds() forming it.
  (d) mesh.reconstruct on the synthetic-weight model against the get_z and the five forward calls it contains (render_path),
      each measured apart in the same run.

    python tools/mesh_time.py [--rounds 5] [--iters 20] [--out profiles/r18_mesh.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from summaries_time import spread, time_form                                          # noqa: E402
from coponerf_amd import _hip, mesh, synthetic as syn                                 # noqa: E402

S, K = 256, 5
BALL_C, BALL_R, WALL_Z = np.array([0.05, -0.03, 3.0]), 0.8, 4.5
LO, HI = (-1.5, -1.5, 1.8), (1.5, 1.5, 4.8)


def analytic_views(dev):
    """render_path's dict for K cameras on an arc about the sphere, and the (1, 4, 4) intrinsics."""
    fx = 0.5 * S / np.tan(np.radians(30.0))
    intr = np.array([[fx, 0, 127.5, 0], [0, fx, 127.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float32)[None]
    v, u = np.divmod(np.arange(S * S), S)
    ray = np.stack(((u - 127.5) / fx, (v - 127.5) / fx, np.ones(S * S)), axis=-1)
    poses, depth = np.zeros((K, 1, 4, 4), dtype=np.float32), np.empty((K, 1, S * S), dtype=np.float32)
    for k, yaw in enumerate(np.radians(np.linspace(-16.0, 16.0, K))):
        c, s = np.cos(yaw), np.sin(yaw)
        R = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])
        pivot = np.array([0.0, 0.0, 3.0])
        poses[k, 0, :3, :3], poses[k, 0, :3, 3], poses[k, 0, 3, 3] = R, pivot - R @ pivot, 1.0
        P = poses[k, 0].astype(np.float64)
        dirs, org = ray @ P[:3, :3].T, P[:3, 3]
        oc = org - BALL_C
        qa, qb, qc = (dirs * dirs).sum(-1), 2.0 * (dirs @ oc), oc @ oc - BALL_R ** 2
        disc = qb * qb - 4.0 * qa * qc
        ball = np.where(disc > 0, (-qb - np.sqrt(np.abs(disc))) / (2.0 * qa), np.inf)
        wall = (WALL_Z - org[2]) / dirs[:, 2]
        depth[k, 0] = np.minimum(ball, wall)                  # lambda . (.., .., 1): the z-depth in the camera
    rgb = np.random.default_rng(18).uniform(-1, 1, size=(K, 1, S * S, 3)).astype(np.float32)
    views = {"depth": torch.from_numpy(depth).to(dev), "valid": torch.ones(K, 1, S * S, dtype=torch.uint8, device=dev),
             "rgb": torch.from_numpy(rgb).to(dev), "poses": torch.from_numpy(poses).to(dev)}
    return views, torch.from_numpy(intr).to(dev)


def stock_integrate(views, intr, origin, spacing, trunc, N):
    """cpn_tsdf_integrate's rule for pair 0 in stock float64 ops: what a user would write without the kernel."""
    dev = intr.device
    o, sp, tr = origin[0].double(), spacing[0].double(), trunc[0].double()
    g = torch.arange(N, device=dev, dtype=torch.float64)
    Z, Y, X = torch.meshgrid(o[2] + g * sp[2], o[1] + g * sp[1], o[0] + g * sp[0], indexing="ij")
    fx, fy, cx, cy = (intr[0, i, j].double() for i, j in ((0, 0), (1, 1), (0, 2), (1, 2)))
    total = torch.zeros_like(X)
    col = torch.zeros(N, N, N, 3, dtype=torch.float64, device=dev)
    n = torch.zeros_like(X)
    for k in range(int(views["depth"].shape[0])):
        P = views["poses"][k, 0].double()
        d = (X - P[0, 3], Y - P[1, 3], Z - P[2, 3])
        Yc = [(P[0, j] * d[0] + P[1, j] * d[1]) + P[2, j] * d[2] for j in range(3)]
        c = torch.floor((fx * Yc[0]) / Yc[2] + cx + 0.5)
        r = torch.floor((fy * Yc[1]) / Yc[2] + cy + 0.5)
        inside = (Yc[2] > 0) & (c >= 0) & (c < S) & (r >= 0) & (r < S)
        at = torch.where(inside, r * S + c, torch.zeros_like(c)).long().reshape(-1)
        dd = views["depth"][k, 0][at].reshape(N, N, N).double()
        s = dd - Yc[2]
        upd = inside & (dd > 0) & (dd < 10) & (views["valid"][k, 0][at].reshape(N, N, N) != 0) & ~(s < -tr)
        total += torch.where(upd, torch.clamp(s / tr, max=1.0), torch.zeros_like(s))
        col += torch.where(upd.unsqueeze(-1), views["rgb"][k, 0][at].reshape(N, N, N, 3).double(), torch.zeros_like(col))
        n += upd
    some = n > 0
    nn = torch.where(some, n, torch.ones_like(n))
    return torch.where(some, total / nn, torch.ones_like(n)).float(), n.to(torch.uint8), (col / nn.unsqueeze(-1)).float()


def measure(forms, rounds, iters):
    """name -> spread of the HIP-event ms per call, the forms alternating within every round."""
    for fn in forms.values():
        time_form(fn, 2)
    ev = {k: [] for k in forms}
    for _ in range(rounds):
        for k, fn in forms.items():
            ev[k].append(time_form(fn, iters)[0])
    return {k: spread(v) for k, v in ev.items()}


def volume_forms(views, intr, N, dev):
    """The forms of one volume size, and what the stock composition and the kernel disagree in."""
    lo, hi = torch.tensor([LO], device=dev), torch.tensor([HI], device=dev)
    vol = mesh.integrate(views, intr, S, dims=(N, N, N), bounds=(lo, hi))
    m = vol.extract()
    cells = (N - 1) ** 3
    lib = _hip.lib()
    scratch = torch.empty(max(lib.cpn_surface_vertices_scratch(1, N, N, N), lib.cpn_surface_faces_scratch(1, N, N, N)),
                          dtype=torch.int32, device=dev)
    cell_vertex = torch.empty(1, cells, dtype=torch.int32, device=dev)
    capv, capf = int(m.xyz.shape[1]), int(m.faces.shape[1])
    st = _hip.stream_handle()

    def kernel():
        _hip.call("cpn_tsdf_integrate", views["depth"].data_ptr(), views["valid"].data_ptr(), views["rgb"].data_ptr(),
                  views["poses"].data_ptr(), intr.data_ptr(), vol.origin.data_ptr(), vol.spacing.data_ptr(), vol.trunc.data_ptr(), K, 1, S,
                  0, 0, S, S, N, N, N, vol.tsdf.data_ptr(), vol.weight.data_ptr(), vol.colour.data_ptr(), st)

    def vertices():
        _hip.call("cpn_surface_vertices", vol.tsdf.data_ptr(), vol.weight.data_ptr(), vol.colour.data_ptr(), vol.origin.data_ptr(),
                  vol.spacing.data_ptr(), 1, N, N, N, 1, capv, scratch.data_ptr(), m.xyz.data_ptr(), m.rgb.data_ptr(), m.nvert.data_ptr(),
                  cell_vertex.data_ptr(), st)

    def faces():
        _hip.call("cpn_surface_faces", vol.tsdf.data_ptr(), cell_vertex.data_ptr(), 1, N, N, N, capf, scratch.data_ptr(),
                  m.faces.data_ptr(), m.nface.data_ptr(), st)

    vertices()
    t, w, c = stock_integrate(views, intr, vol.origin, vol.spacing, vol.trunc, N)
    agree = {"voxels": N ** 3, "updated_voxels": int((vol.weight > 0).sum()), "weight_differs": int((w != vol.weight[0]).sum()),
             "tsdf_bits_differ": int((t.view(torch.int32) != vol.tsdf[0].view(torch.int32)).sum()),
             "colour_bits_differ": int((c.view(torch.int32) != vol.colour[0].view(torch.int32)).sum()),
             "vertices": int(m.nvert[0]), "triangles": int(m.nface[0]), "max_vertices": capv, "max_faces": capf}
    del t, w, c
    forms = {"cpn_tsdf_integrate": kernel,
             "stock_ops_integrate_float64": lambda: stock_integrate(views, intr, vol.origin, vol.spacing, vol.trunc, N),
             "cpn_surface_vertices": vertices, "cpn_surface_faces": faces,
             "integrate_extract_box_given": lambda: mesh.integrate(views, intr, S, dims=(N, N, N), bounds=(lo, hi)).extract(),
             "integrate_extract_with_bounds": lambda: mesh.integrate(views, intr, S, dims=(N, N, N)).extract()}
    return forms, agree


def model_forms(dev):
    from coponerf_amd import CoPoNeRF
    from coponerf_amd.novel_views import prepare_pair, render_path
    model = CoPoNeRF.CoPoNeRF(n_view=2)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(syn.make_full_weights(shapes), strict=True)
    model = model.to(dev).eval()
    frames = syn.make_scene(n=2)[0]
    inp = prepare_pair(frames[0], frames[1], hfov_deg=75.0, device=dev)
    t = (0.0, 0.25, 0.5, 0.75, 1.0)
    with torch.no_grad():
        views = render_path(model, inp, t, return_rgb=True, return_depth=True)
    Kq = inp["query"]["intrinsics"]

    def get_z():
        with torch.no_grad():
            model.get_z(inp)

    return {"get_z": get_z,
            "render_path_5_views (get_z + 5 forward)": lambda: render_path(model, inp, t, return_rgb=True, return_depth=True),
            "mesh.reconstruct_128 (render_path + integrate + extract)": lambda: mesh.reconstruct(model, inp, t),
            "integrate_extract_128_of_those_views": lambda: mesh.integrate(views, Kq, S).extract()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--model-iters", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mesh_time.py measures on a HIP device"
    dev = torch.device("cuda:0")
    views, intr = analytic_views(dev)
    res = {"device": torch.cuda.get_device_name(0), "views": f"{K} analytic views of {S} x {S}, one pair", "iters": a.iters,
           "rounds": a.rounds, "unit": "ms per call, HIP events, median / min / max of the rounds", "volumes": {}}
    for N in (128, 256):
        forms, agree = volume_forms(views, intr, N, dev)
        res["volumes"][f"{N}^3"] = {"agreement_kernel_vs_stock_ops": agree, "ms": measure(forms, a.rounds, a.iters)}
        del forms
        torch.cuda.empty_cache()
    res["model"] = {"iters": a.model_iters, "ms": measure(model_forms(dev), a.rounds, a.model_iters)}
    res["note"] = ("extraction has no stock-op composition without a host read, so none is timed; the stock-op integrate is float64 on "
                   "the device in the kernel's operation order; the model carries synthetic weights (no trained checkpoint is available), "
                   "so its depth maps are noise and the mesh of (d) is whatever that gives - the time of integrate does not depend on "
                   "the values, that of the extraction grows with the number of active cells")
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
