"""What a view of the point cloud costs (coponerf_amd/splat.py), on one MI355X, in one process.

The cloud is fixed by construction: a tilted plane seen by two 256 x 256 cameras (the identity, and one turned 4 degrees and
moved 0.3 units), every pixel unprojected (cpn_depth_points) and kept (cpn_compact_points): 131 072 points with seeded random
colours.  It is drawn into K = 60 orbit cameras (orbit_poses: pivot at the plane's depth on the axis, +-30 degrees) at
256 x 256 and radius 1.

  (a) cpn_splat_points (its clear and its launch), cpn_splat_resolve and cpn_splat_score (its two launches), each by HIP
      events, the median of --iters calls;
  (b) `draw` as a whole (both entry points and the allocations; no host read) against the same result composed from stock
      operators: the projection in float64 torch element-wise operations in the kernel's order, scatter_reduce_(..., "amin")
      on int64 keys into a (K B H W) buffer for each of the nine footprint offsets, and an indexed gather of the colours.  Its
      index image is compared with draw's before anything is timed, and the number of pixels that differ is recorded.  Both by
      wall clock around a synchronise, in alternating windows of --reps calls of draw and --stock-reps of the composition;
      every window is kept;
  (c) for context, render_path's time per 256 x 256 frame of the synthetic-weight model in the same process (4 frames a call).

There is no pass / fail time: the numbers are recorded, and (a), (b), (c) are compared within this run only.

    python tools/splat_time.py [--rounds 6] [--reps 200] [--stock-reps 2] [--iters 50] [--out profiles/r17_splat.json]
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
from coponerf_amd import CoPoNeRF, _hip, novel_views as nv, point_cloud as pc, splat, synthetic as syn   # noqa: E402

S = 256
K_ORBIT = 60
PIVOT_Z, YAW_DEG = 4.0, 30.0
RADIUS = 1


def wall(fn, reps):
    """ms per call of `reps` calls between two synchronises."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


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


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def plane_cloud(dev):
    """The cloud of the docstring and its (1, 4, 4) intrinsics (75 degrees across, the principal point at the centre)."""
    f = (S / 2.0) / np.tan(np.radians(75.0 / 2.0))
    Kb = torch.tensor([[f, 0, S / 2.0, 0], [0, f, S / 2.0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=torch.float32).view(1, 4, 4).to(dev)
    a = np.radians(4.0)
    P = np.tile(np.eye(4), (2, 1, 1, 1))
    P[1, 0, :3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
    P[1, 0, :3, 3] = [0.3, 0.05, -0.1]
    P32 = P.astype(np.float32)
    n, c = np.array([-0.3, -0.2, 1.0]), PIVOT_Z                      # the plane z = 4 + 0.3 x + 0.2 y
    K64 = Kb[0].cpu().numpy().astype(np.float64)
    v, u = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64), indexing="ij")
    ray = np.stack(((u - K64[0, 2]) / K64[0, 0], (v - K64[1, 2]) / K64[1, 1], np.ones_like(u)), axis=-1).reshape(-1, 3)
    depth = np.stack([(c - P32[k, 0, :3, 3].astype(np.float64) @ n) / ((ray @ P32[k, 0, :3, :3].astype(np.float64).T) @ n)
                      for k in range(2)]).astype(np.float32).reshape(2, 1, S * S)
    depth_d, poses_d = torch.from_numpy(depth).to(dev), torch.from_numpy(P32).to(dev)
    xyz = pc.unproject(depth_d, poses_d, Kb, S)
    rgb = torch.from_numpy(np.random.default_rng(17).uniform(-1, 1, size=(2, 1, S * S, 3)).astype(np.float32)).to(dev)
    cloud = pc.compact(torch.ones(2, 1, S * S, dtype=torch.uint8, device=dev), xyz, rgb, S, S)
    return cloud, Kb


def stock(cloud, poses, Kb, H, W, radius, near=1e-3):
    """draw(..., return_index=True) from stock operators -> (frames (K, B, H, W, 3) uint8, index (K, B, H, W) int32).  The
    geometry in float64 element-wise operations in the kernel's order (no matrix product: its sums run in another order);
    the cameras' own finiteness is not tested."""
    xyz, rgb, count = cloud.xyz, cloud.rgb, cloud.count
    B, cap = int(xyz.shape[0]), int(xyz.shape[1])
    K, dev = int(poses.shape[0]), xyz.device
    X, P, Km = xyz.double(), poses.double(), Kb.double()
    d = [X[None, :, :, a] - P[:, :, a, 3, None] for a in range(3)]
    Y = [(P[:, :, 0, j, None] * d[0] + P[:, :, 1, j, None] * d[1]) + P[:, :, 2, j, None] * d[2] for j in range(3)]
    u = (Km[None, :, 0, 0, None] * Y[0]) / Y[2] + Km[None, :, 0, 2, None]
    v = (Km[None, :, 1, 1, None] * Y[1]) / Y[2] + Km[None, :, 1, 2, None]
    z32 = Y[2].float()
    i = torch.arange(cap, device=dev)
    ok = (i[None, None, :] < count.clamp(0, cap)[None, :, None]) & torch.isfinite(X).all(dim=-1)[None] & (Y[2] >= near) & \
        (u.abs() < 2.0 ** 30) & (v.abs() < 2.0 ** 30) & torch.isfinite(z32)
    c = torch.where(ok, torch.floor(u + 0.5), torch.zeros_like(u)).long()
    r = torch.where(ok, torch.floor(v + 0.5), torch.zeros_like(v)).long()
    key = ((z32.view(torch.int32).long() << 32) | i[None, None, :]).reshape(-1)         # z32 >= 0: the sign bit is clear
    n = K * B * H * W
    empty = torch.iinfo(torch.int64).max
    zb = torch.full((n + 1,), empty, dtype=torch.int64, device=dev)                      # one more slot: the clipped pixels'
    base = torch.arange(K * B, device=dev).view(K, B, 1) * (H * W)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            rr, cc = r + dy, c + dx
            inside = ok & (rr >= 0) & (rr < H) & (cc >= 0) & (cc < W)
            at = torch.where(inside, base + rr * W + cc, torch.full_like(rr, n))
            zb.scatter_reduce_(0, at.reshape(-1), key, "amin")
    zb = zb[:n].view(K, B, H, W)
    hit = zb != empty
    index = torch.where(hit, zb & 0xFFFFFFFF, torch.full_like(zb, -1))
    pair = torch.arange(B, device=dev).view(1, B, 1, 1).expand(K, B, H, W)
    frames = rgb[pair, index.clamp(min=0)] * hit[..., None].to(torch.uint8)
    return frames, index.int()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--stock-reps", type=int, default=2)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)

    cloud, Kb = plane_cloud(dev)
    B, cap = int(cloud.xyz.shape[0]), int(cloud.xyz.shape[1])
    poses = splat.orbit_poses(B, K_ORBIT, PIVOT_Z, YAW_DEG, device=dev)
    K = K_ORBIT
    res = {"device": torch.cuda.get_device_name(dev), "arch": torch.cuda.get_device_properties(dev).gcnArchName, "cameras": K, "pairs": B, "side": S, "radius": RADIUS, "cap": cap,
           "points": int(cloud.count[0]), "rounds": args.rounds, "reps": args.reps, "stock_reps": args.stock_reps, "iters": args.iters}

    # ---- (a) the entry points by events
    zbuf = torch.empty(K, B, S, S, dtype=torch.int64, device=dev)
    frames = torch.empty(K, B, S, S, 3, dtype=torch.uint8, device=dev)
    depth = torch.empty(K, B, S, S, dtype=torch.float32, device=dev)
    index = torch.empty(K, B, S, S, dtype=torch.int32, device=dev)
    target = torch.from_numpy(np.random.default_rng(18).integers(0, 256, size=(K, B, S, S, 3), dtype=np.uint8)).to(dev)
    scratch = torch.empty(_hip.lib().cpn_splat_score_scratch(K, B, S, S), dtype=torch.int64, device=dev)
    stats = torch.empty(K, B, 2, dtype=torch.int64, device=dev)
    stream = _hip.stream_handle()
    kern = {}
    kern["splat_points_ms"] = events(lambda: _hip.call("cpn_splat_points", cloud.xyz.data_ptr(), cloud.count.data_ptr(), poses.data_ptr(),
                                                       Kb.data_ptr(), K, B, cap, S, S, RADIUS, 1e-3, zbuf.data_ptr(), stream), args.iters)
    kern["splat_resolve_ms"] = events(lambda: _hip.call("cpn_splat_resolve", zbuf.data_ptr(), cloud.rgb.data_ptr(), K, B, cap, S, S, 0, 0,
                                                        frames.data_ptr(), depth.data_ptr(), index.data_ptr(), stream), args.iters)
    kern["splat_resolve_fill1_ms"] = events(lambda: _hip.call("cpn_splat_resolve", zbuf.data_ptr(), cloud.rgb.data_ptr(), K, B, cap, S, S,
                                                              1, 0, frames.data_ptr(), depth.data_ptr(), index.data_ptr(), stream),
                                            args.iters)
    kern["splat_score_ms"] = events(lambda: _hip.call("cpn_splat_score", frames.data_ptr(), index.data_ptr(), target.data_ptr(), K, B, S,
                                                      S, scratch.data_ptr(), stats.data_ptr(), stream), args.iters)
    res["entry_points"] = kern
    res["covered_share"] = float((index >= 0).float().mean())

    # ---- (b) draw against the stock composition, checked first
    ours = lambda: splat.draw(cloud, poses, Kb, S, S, radius=RADIUS, return_index=True)
    theirs = lambda: stock(cloud, poses, Kb, S, S, RADIUS)
    mine, (s_frames, s_index) = ours(), theirs()
    res["stock_check"] = {"pixels": int(s_index.numel()), "index_pixels_that_differ": int((mine["index"] != s_index).sum()),
                          "frame_bytes_that_differ": int((mine["frames"] != s_frames).sum())}
    del mine, s_frames, s_index
    for fn in (ours, theirs):
        fn()
    runs = {"draw_ms": [], "stock_ops_ms": []}
    for _ in range(args.rounds):                               # alternating windows
        runs["draw_ms"].append(wall(ours, args.reps))
        runs["stock_ops_ms"].append(wall(theirs, args.stock_reps))
    res.update(runs)
    res["draw_ms_per_frame"] = spread([t / K for t in runs["draw_ms"]])

    # ---- (c) a network frame, for context
    model = CoPoNeRF.CoPoNeRF(n_view=2)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(syn.make_full_weights(shapes), strict=True)
    model = model.to(dev).eval()
    photos = syn.make_scene(n=2)[0]
    inp = nv.prepare_pair(photos[0], photos[1], hfov_deg=75.0, device=dev)
    ts = (0.2, 0.4, 0.6, 0.8)
    path = lambda: nv.render_path(model, inp, ts)
    path()
    path()
    res["render_path_ms_per_frame"] = [wall(path, 2) / len(ts) for _ in range(args.rounds)]
    res["summary"] = {k: spread(res[k]) for k in ("draw_ms", "stock_ops_ms", "render_path_ms_per_frame")}

    print(json.dumps(res, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
