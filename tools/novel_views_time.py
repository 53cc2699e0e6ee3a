"""What a view sequence costs (coponerf_amd/novel_views.py), on one MI355X.

  (a) ms per frame of a K = 16 full-image path of one 256 x 256 pair through `render_path` - the wall time of the call less
      that of its `get_z`, over K - with every next camera announced (CoPoNeRF.prepare_next) and with that switched off,
      against bench.py's default headline loop restated here (one full-image forward(val=True) per step on the same cached
      cameras, one stream): four alternating runs of each in this process, wall clock around a synchronise.
      Expected: a frame costs the headline's per-image time plus the pack kernel, within the headline's own spread.
  (b) the three kernels of csrc/novel_views.hip by HIP events: cpn_fit_images_u8 at 360 x 640 -> 256 and at 4000 x 6000 -> 256
      (two views), cpn_camera_path at K = 16, cpn_pack_frames of one 256 x 256 frame with and without the depth panel.
  (c) the engine's contractual `pixel_val` copy of one frame (8 N R S bytes to pinned host memory) by HIP events.

    python tools/novel_views_time.py [--frames 16] [--rounds 4] [--iters 50] [--out profiles/r12_novel_views.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from coponerf_amd import CoPoNeRF, novel_views as nv, synthetic as syn   # noqa: E402

S = 256


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def events(fn, iters):
    """Median ms of fn() between two HIP events."""
    fn()
    times = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    K = args.frames

    model = CoPoNeRF.CoPoNeRF(n_view=2)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(syn.make_full_weights(shapes), strict=True)
    model = model.to(dev).eval()
    frames = syn.make_scene(n=2)[0]
    inp = nv.prepare_pair(frames[0], frames[1], hfov_deg=75.0, device=dev)
    ts = np.linspace(0.0, 1.0, K)

    # bench.py's headline loop: one full-image call per step, the same cameras and latents every step, one stream
    with torch.no_grad():
        z, rel, flow = model.get_z(inp)
    head_inp = {"context": inp["context"], "query": dict(inp["query"], cam2world=rel.unsqueeze(1).contiguous())}

    def headline():
        with torch.no_grad():
            for _ in range(K):
                model(head_inp, z=z, rel_pose=rel, val=True, flow=flow)

    def get_z():
        with torch.no_grad():
            model.get_z(inp)

    lanes = model._engine.call_lanes
    model._engine.call_lanes = 1
    forms = {"headline": headline, "get_z": get_z,
             "path": lambda: nv.render_path(model, inp, ts),
             "path_unannounced": lambda: nv.render_path(model, inp, ts, announce=False)}
    for fn in forms.values():                              # warm-up: workspaces, pinned buffers, packed weights
        fn()
        fn()
    runs = {name: [] for name in forms}
    for _ in range(args.rounds):                           # alternating
        for name, fn in forms.items():
            runs[name].append(wall(fn))
    model._engine.call_lanes = lanes
    per = lambda name: [(t - g) / K for t, g in zip(runs[name], runs["get_z"])]
    res = {"frames": K, "rounds": args.rounds,
           "headline_ms_per_image": [t / K for t in runs["headline"]], "get_z_ms": runs["get_z"],
           "path_ms_per_frame": per("path"), "path_unannounced_ms_per_frame": per("path_unannounced")}
    med = lambda v: statistics.median(v)
    res["median"] = {k: med(res[k]) for k in ("headline_ms_per_image", "get_z_ms", "path_ms_per_frame", "path_unannounced_ms_per_frame")}
    res["headline_spread_ms"] = max(res["headline_ms_per_image"]) - min(res["headline_ms_per_image"])

    # ---- (b) the kernels
    kern = {}
    for name, (Hi, Wi) in (("fit_360x640", (360, 640)), ("fit_4000x6000", (4000, 6000))):
        a = torch.randint(0, 256, (2, Hi, Wi, 3), dtype=torch.uint8, device=dev)
        out = torch.empty(1, 2, S, S, 3, device=dev)
        kern[name + "_ms"] = events(lambda: nv.fit_images(a[:1], a[1:], out, True), args.iters)
    rel16 = rel.expand(1, 4, 4).contiguous()
    td = torch.linspace(0, 1, K, dtype=torch.float64, device=dev)
    kern["camera_path_ms"] = events(lambda: nv.camera_path(rel16, td, sway=0.02), args.iters)
    rgb = torch.rand(1, S * S, 3, device=dev) * 2 - 1
    depth = torch.rand(1, S * S, device=dev) * 10
    f1 = torch.empty(1, S, S, 3, dtype=torch.uint8, device=dev)
    f2 = torch.empty(1, S, 2 * S, 3, dtype=torch.uint8, device=dev)
    kern["pack_frames_ms"] = events(lambda: nv.pack_frames(rgb, f1), args.iters)
    kern["pack_frames_depth_ms"] = events(lambda: nv.pack_frames(rgb, f2, depth), args.iters)
    res["kernels"] = kern

    # ---- (c) the pixel_val copy of one frame: (N, R, S, 2) fp32 to pinned memory
    pv = torch.empty(2, S * S, model.npoints, 2, device=dev)
    host = torch.empty(pv.shape, dtype=torch.float32, pin_memory=True)
    res["pixel_val_copy_ms"] = events(lambda: host.copy_(pv, non_blocking=True), args.iters)
    res["pixel_val_bytes"] = pv.numel() * 4

    print(json.dumps(res, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
