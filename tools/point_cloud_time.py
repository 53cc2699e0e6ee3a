"""What a point cloud costs (coponerf_amd/point_cloud.py), on one MI355X, in one process.

  (a) the three kernels of csrc/point_cloud.hip on two full 256 x 256 views of one pair - cpn_depth_votes, cpn_depth_points,
      cpn_compact_points - by HIP events, and `from_views` (the three, the mask between them and their allocations; no host
      read) by wall clock around a synchronise.  Two inputs: `rendered`, the views t = 0, 1 as render_path returns them for
      the synthetic weights (these carry no geometry: a third of the depths are valid and none agrees across the views), and
      `plane`, the depth of a tilted plane ray-cast here for the identity and a camera 4 degrees and 0.3 units away, with the
      pair's intrinsics and the rendered colours (nearly every pixel that sees the other view votes).
  (b) the same result composed from stock operators in float64: torch matrix products for the geometry, F.grid_sample
      (bilinear, align_corners=True) for the depth lookup and for the all-four-taps-valid test, boolean indexing for the
      compaction - which reads the host, so it is timed by wall clock around a synchronise, like `from_views`.  Its votes are
      compared with the kernel's and the number of differing pixels is recorded (grid_sample forms its weights in another
      order, so a decision next to a threshold may differ).
  (c) `reconstruct` of the pair against what it contains: get_z and the two forward(val=True) calls (bench.py's headline
      loop restated: the same cached cameras, one stream), alternating rounds, wall clock.

There is no pass / fail time: the numbers are recorded, and (a) is compared with (b) from the same run only.

    python tools/point_cloud_time.py [--rounds 4] [--iters 50] [--out profiles/r15_point_cloud.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from coponerf_amd import CoPoNeRF, _hip, novel_views as nv, point_cloud as pc, synthetic as syn   # noqa: E402

S = 256
TS = (0.0, 1.0)


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


def stock(depth, valid, rgb, poses, intr, px_tol=1.0, rel_tol=0.01):
    """from_views(fuse=True, min_votes=1) of full S x S views from stock operators, float64: (xyz (n, 3), rgb (n, 3), votes)."""
    K, B, R = depth.shape
    dev = depth.device
    d = depth.double()
    P = poses.double()
    fx, fy, cx, cy = (intr[:, i, j].double().view(B, 1) for i, j in ((0, 0), (1, 1), (0, 2), (1, 2)))
    ar = torch.arange(S, dtype=torch.float64, device=dev)
    u, v = ar.repeat(S).view(1, R), ar.repeat_interleave(S).view(1, R)
    ok = torch.isfinite(d) & (d > 0) & (d < 10)

    def lift(dd, uu, vv, k):                               # pose_k . (d . ray)
        p = torch.stack((dd * (uu - cx) / fx, dd * (vv - cy) / fy, dd), dim=-1)
        return p @ P[k, :, :3, :3].transpose(1, 2) + P[k, :, None, :3, 3]

    def lower(X, k):                                       # pose_k^-1 X and its pixel
        Y = (X - P[k, :, None, :3, 3]) @ P[k, :, :3, :3]
        return Y, fx * Y[..., 0] / Y[..., 2] + cx, fy * Y[..., 1] / Y[..., 2] + cy

    votes = torch.zeros(K, B, R, dtype=torch.uint8, device=dev)
    total = torch.where(ok, d, torch.zeros_like(d))
    maps = torch.where(ok, d, torch.zeros_like(d)).view(K, B, 1, S, S)
    okmaps = ok.double().view(K, B, 1, S, S)
    for a in range(K):
        X = lift(torch.where(ok[a], d[a], torch.ones_like(d[a])), u, v, a)
        for b in range(K):
            if b == a:
                continue
            Y, qx, qy = lower(X, b)
            grid = torch.stack((2 * qx / (S - 1) - 1, 2 * qy / (S - 1) - 1), dim=-1).view(B, 1, R, 2)
            db = F.grid_sample(maps[b], grid, mode="bilinear", align_corners=True).view(B, R)
            allok = F.grid_sample(okmaps[b], grid, mode="bilinear", align_corners=True).view(B, R) > 1 - 1e-9
            inside = (Y[..., 2] > 0) & (qx >= 0) & (qx < S - 1) & (qy >= 0) & (qy < S - 1) & allok
            Y2, bx, by = lower(lift(db, qx, qy, b), a)
            yes = ok[a] & inside & (Y2[..., 2] > 0) & (torch.hypot(bx - u, by - v) <= px_tol) & \
                ((Y2[..., 2] - d[a]).abs() <= rel_tol * d[a])
            votes[a] += yes.to(torch.uint8)
            total[a] = total[a] + torch.where(yes, Y2[..., 2], torch.zeros_like(d[a]))
    fused = torch.where(ok, total / (1 + votes.double()), torch.full_like(d, float("nan"))).float()
    xyz = torch.stack([lift(fused[k].double(), u, v, k) for k in range(K)]).float()
    keep = (fused > 0) & (fused < 10) & (votes >= 1) & (valid != 0)
    out_xyz = xyz.transpose(0, 1)[keep.transpose(0, 1)]                            # boolean indexing: the host read
    out_rgb = ((rgb.transpose(0, 1)[keep.transpose(0, 1)] + 1) * 127.5).clamp(0, 255).round().to(torch.uint8)
    return out_xyz, out_rgb, votes


def plane_views(views, Kb):
    """`views` with the depth of the plane z = 4 + 0.3 x + 0.2 y seen from the identity and from a camera turned 4 degrees about
    y and moved by (0.3, 0.05, -0.1): float64 ray casting, rounded to fp32 once."""
    dev = Kb.device
    B = Kb.shape[0]
    a = torch.deg2rad(torch.tensor(4.0, dtype=torch.float64))
    P = torch.eye(4, dtype=torch.float64).repeat(2, B, 1, 1)
    P[1, :, :3, :3] = torch.tensor([[torch.cos(a), 0, torch.sin(a)], [0, 1, 0], [-torch.sin(a), 0, torch.cos(a)]], dtype=torch.float64)
    P[1, :, :3, 3] = torch.tensor([0.3, 0.05, -0.1], dtype=torch.float64)
    P = P.float().to(dev)
    n, c = torch.tensor([-0.3, -0.2, 1.0], dtype=torch.float64, device=dev), 4.0
    ar = torch.arange(S, dtype=torch.float64, device=dev)
    u, v = ar.repeat(S).view(1, -1), ar.repeat_interleave(S).view(1, -1)
    K64 = Kb.double()
    ray = torch.stack(((u - K64[:, 0, 2:3]) / K64[:, 0, 0:1], (v - K64[:, 1, 2:3]) / K64[:, 1, 1:2], torch.ones_like(u).expand(B, -1)), dim=-1)
    depth = torch.stack([(c - P[k, :, :3, 3].double() @ n)[:, None] / ((ray @ P[k, :, :3, :3].double().transpose(1, 2)) @ n) for k in range(2)])
    return dict(views, depth=depth.float().contiguous(), poses=P.contiguous(), valid=torch.ones_like(views["valid"]))


def kernels_and_stock(views, Kq, Kb, args):
    """(a) and (b) of the module's docstring on one set of views."""
    depth, poses, rgb, valid = views["depth"], views["poses"], views["rgb"], views["valid"]
    K, B, R = depth.shape
    dev = depth.device
    res = {"valid_depth_share": float(((depth > 0) & (depth < 10)).float().mean())}
    votes = torch.empty(K, B, R, dtype=torch.uint8, device=dev)
    fused = torch.empty(K, B, R, dtype=torch.float32, device=dev)
    xyz = torch.empty(K, B, R, 3, dtype=torch.float32, device=dev)
    stream = _hip.stream_handle()
    kern = {}
    kern["depth_votes_ms"] = events(lambda: _hip.call("cpn_depth_votes", depth.data_ptr(), poses.data_ptr(), Kb.data_ptr(), K, B, S, 0,
                                                      0, S, S, 1.0, 0.01, votes.data_ptr(), fused.data_ptr(), stream), args.iters)
    kern["depth_points_ms"] = events(lambda: _hip.call("cpn_depth_points", fused.data_ptr(), poses.data_ptr(), Kb.data_ptr(), K, B, S,
                                                       0, 0, S, S, xyz.data_ptr(), stream), args.iters)
    keep = ((fused > 0) & (fused < 10) & (votes >= 1) & (valid != 0)).to(torch.uint8)
    out = (torch.empty(B, K * R, 3, device=dev), torch.empty(B, K * R, 3, dtype=torch.uint8, device=dev),
           torch.empty(B, dtype=torch.int32, device=dev))
    scratch = torch.empty(_hip.lib().cpn_compact_points_scratch(K, B, S, S), dtype=torch.int32, device=dev)
    kern["compact_points_ms"] = events(lambda: _hip.call("cpn_compact_points", keep.data_ptr(), xyz.data_ptr(), rgb.data_ptr(), K, B, S,
                                                         S, scratch.data_ptr(), out[0].data_ptr(), out[1].data_ptr(),
                                                         out[2].data_ptr(), stream), args.iters)
    res["kernels"] = kern

    ours = lambda: pc.from_views(views, Kq, S)
    theirs = lambda: stock(depth, valid, rgb, poses, Kb)
    for fn in (ours, theirs):
        fn()
        fn()
    runs = {"from_views_ms": [], "stock_ops_ms": []}
    for _ in range(args.rounds):                           # alternating
        runs["from_views_ms"].append(wall(ours))
        runs["stock_ops_ms"].append(wall(theirs))
    res.update(runs)
    res["median"] = {k: statistics.median(v) for k, v in runs.items()}
    cloud, (s_xyz, s_rgb, s_votes) = ours(), theirs()
    n = int(cloud.count[0])
    res["points"] = {"from_views": n, "stock_ops": int(s_xyz.shape[0]), "pixels": K * B * R,
                     "pixels_with_other_votes": int((pc.vote(depth, poses, Kq, S, 1.0, 0.01)[0] != s_votes).sum())}
    if n == int(s_xyz.shape[0]):
        res["points"]["largest_xyz_difference"] = float((cloud.xyz[0, :n] - s_xyz).abs().max()) if n else 0.0
        res["points"]["colour_bytes_that_differ"] = int((cloud.rgb[0, :n] != s_rgb).sum())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")

    model = CoPoNeRF.CoPoNeRF(n_view=2)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(syn.make_full_weights(shapes), strict=True)
    model = model.to(dev).eval()
    frames = syn.make_scene(n=2)[0]
    inp = nv.prepare_pair(frames[0], frames[1], hfov_deg=75.0, device=dev)
    Kq = inp["query"]["intrinsics"]
    Kb = Kq[:, 0].contiguous()
    views = nv.render_path(model, inp, TS, return_rgb=True, return_depth=True)
    K, B, R = views["depth"].shape
    res = {"views": K, "pairs": B, "side": S, "rounds": args.rounds, "iters": args.iters}

    for name, vw in (("rendered", views), ("plane", plane_views(views, Kb))):
        res[name] = kernels_and_stock(vw, Kq, Kb, args)

    # ---- (c) reconstruct against what it contains
    with torch.no_grad():
        z, rel, flow = model.get_z(inp)
    head_inp = {"context": inp["context"], "query": dict(inp["query"], cam2world=rel.unsqueeze(1).contiguous())}

    def forwards():
        with torch.no_grad():
            for _ in range(K):
                model(head_inp, z=z, rel_pose=rel, val=True, flow=flow)

    def get_z():
        with torch.no_grad():
            model.get_z(inp)

    lanes = model._engine.call_lanes
    model._engine.call_lanes = 1
    forms = {"two_forwards_ms": forwards, "get_z_ms": get_z, "reconstruct_ms": lambda: pc.reconstruct(model, inp, TS)}
    for fn in forms.values():
        fn()
        fn()
    whole = {name: [] for name in forms}
    for _ in range(args.rounds):
        for name, fn in forms.items():
            whole[name].append(wall(fn))
    model._engine.call_lanes = lanes
    res.update(whole)
    res["median"] = {k: statistics.median(res[k]) for k in ("two_forwards_ms", "get_z_ms", "reconstruct_ms")}
    res["median"]["reconstruct_less_its_renders_ms"] = res["median"]["reconstruct_ms"] - res["median"]["get_z_ms"] - \
        res["median"]["two_forwards_ms"]

    print(json.dumps(res, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
