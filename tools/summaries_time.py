"""What the validation log costs (coponerf_amd/summaries.py), on one MI355X.

  (a) one batch of two 256 x 256 pairs through `SummaryLog(lag=1).add` (csrc/summaries.hip + the stock grid ops + one
      asynchronous copy; the entry of the call before is written to a writer that drops it) against the reference's
      composition restated on the device WITH its host traffic (summary/summaries.py:106-235: F.interpolate, grid_sample with
      its grid built on the host, a `.cpu().numpy()` per image and direction for the mask overlay, the depth map through the
      host for the colour map, a `.cpu().numpy()` per grid, a host read per scalar) - alternating in one process, by HIP
      events and by wall clock around a synchronise.  The epipolar drawings and the overlay's contour are in neither form.
  (b) wall time per batch of `pipeline.render_images` over `--pairs` batches of two 256 x 256 images: alone, with
      `SummaryLog(lag=1)`, and with the reference-style composition after every render.
  (c) kernel launches of one call of both forms: this script runs itself with `--trace-form` under
      `rocprofv3 --kernel-trace` for 2 and for 12 calls of a form and divides the difference of the traces' rows by 10
      (one-off kernels - building the inputs - cancel).

    python tools/summaries_time.py [--pairs 8] [--rounds 5] [--iters 50] [--out profiles/r10_summaries.json]
"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from coponerf_amd import CoPoNeRF, synthetic as syn                     # noqa: E402
from coponerf_amd.pipeline import render_images                         # noqa: E402
from coponerf_amd.summaries import SummaryLog, jet_table, make_grid     # noqa: E402

S = 256


class DroppingWriter:
    """Takes what a SummaryWriter takes and keeps nothing; a tensor scalar is read as TensorBoard reads it."""

    def add_image(self, tag, img, step):
        assert isinstance(img, np.ndarray)

    def add_scalar(self, tag, value, step):
        float(value)


def _warp(x, flo):
    """utils_training/utils.py:642-671 as written: the pixel grid is built on the host and copied over on every call."""
    B, C, H, W = x.size()
    xx = torch.arange(0, W).view(1, -1).repeat(H, 1).view(1, 1, H, W).repeat(B, 1, 1, 1)
    yy = torch.arange(0, H).view(-1, 1).repeat(1, W).view(1, 1, H, W).repeat(B, 1, 1, 1)
    vgrid = torch.cat((xx, yy), 1).float().to(flo.device) + flo
    vgrid[:, 0] = 2.0 * vgrid[:, 0].clone() / max(W - 1, 1) - 1.0
    vgrid[:, 1] = 2.0 * vgrid[:, 1].clone() / max(H - 1, 1) - 1.0
    return F.grid_sample(x, vgrid.permute(0, 2, 3, 1), align_corners=False)


def _inside(flow):
    B, _, H, W = flow.shape
    xx = torch.arange(0, W).view(1, -1).repeat(H, 1).view(1, 1, H, W).repeat(B, 1, 1, 1)
    yy = torch.arange(0, H).view(-1, 1).repeat(1, W).view(1, 1, H, W).repeat(B, 1, 1, 1)
    m = flow + torch.cat((xx, yy), 1).float().to(flow.device)
    return m[:, 0].ge(0) & m[:, 0].le(W - 1) & m[:, 1].ge(0) & m[:, 1].le(H - 1)


def _overlay(im, ann, color=(255, 102, 51), alpha=0.5):
    """summaries.py:42-63 on the host, without the contour."""
    im, ann = np.asarray(im, dtype=np.uint8), np.asarray(ann, dtype=np.uint8)
    fg = im * alpha + (1 - alpha) * np.asarray(color, dtype=np.uint8)
    img = im.copy()
    img[ann > 0] = fg[ann > 0]
    return img


def reference_style(model_input, model_output, writer, step, table):
    """summaries.py:106-235 on device tensors with the host traffic of the original."""
    grid = lambda t, **kw: make_grid(t, **kw).cpu().numpy()
    predictions = model_output["rgb"].view(-1, S, S, 3).permute(0, 3, 1, 2).clamp(-1, 1)
    at_wt = model_output["at_wt"]
    ent = (-(at_wt * torch.log(at_wt + 1e-5)).sum(dim=-1)).mean()
    writer.add_scalar("ent", ent, step)
    bool(torch.isnan(ent))
    writer.add_image("predictions", grid(predictions), step)
    depth = model_output["depth_ray"].view(-1, S, S).detach().cpu().numpy() / 10.
    x = depth * np.float32(256)
    with np.errstate(invalid="ignore"):
        idx = np.where(x < 0, 0, np.where(x >= 256, 255, x.astype(np.int64)))
    colours = table[np.where(np.isnan(x), 0, idx)]
    colours[np.isnan(x)] = 0.0
    writer.add_image("depth_images", grid(torch.Tensor(colours.transpose(0, 3, 1, 2)), scale_each=True), step)
    ctx = model_input["context"]["rgb"]
    writer.add_image("context_images", grid(ctx.flatten(0, 1).permute(0, 3, 1, 2)), step)
    query = model_input["query"]["rgb"].view(-1, S, S, 3).permute(0, 3, 1, 2)
    writer.add_image("query_images", grid(query), step)
    h = model_output["flow"][0].shape[2]
    flow = F.interpolate(model_output["flow"][0], S, mode="bilinear") * (S / h)
    flow2 = F.interpolate(model_output["flow"][1], S, mode="bilinear") * (S / h)
    mask = torch.norm(flow + _warp(flow2, flow), dim=1).le(10) * _inside(flow)
    mask2 = torch.norm(flow2 + _warp(flow, flow2), dim=1).le(10) * _inside(flow2)
    for fl, mk, src, suffix in ((flow, mask, 1, ""), (flow2, mask2, 0, "_flip")):
        warped, overlaid = [], []
        for i in range(len(fl)):
            temp = _warp((ctx[i, src].permute(2, 0, 1).unsqueeze(0) + 1) * 127.5, fl[i]).squeeze(0).permute(1, 2, 0)
            warped.append(temp)
            overlaid.append(_overlay(temp.cpu().numpy(), 255 - mk[i].cpu().numpy() * 255))
        warped = torch.stack(warped)
        warped = torch.cat(((ctx[:, src] + 1) * 127.5, warped, (ctx[:, 1 - src] + 1) * 127.5), dim=-2)
        writer.add_image("warped_img" + suffix, grid(warped.permute(0, 3, 1, 2)), step)
        writer.add_image("masked_warped_img" + suffix, grid(torch.from_numpy(np.stack(overlaid)).float().permute(0, 3, 1, 2)), step)
    writer.add_scalar("flow_mean", flow.flatten(-2, -1).mean(-1)[0, 0], step)
    writer.add_scalar("out_min", predictions.min(), step)
    writer.add_scalar("out_max", predictions.max(), step)
    rel, gt_rel = model_output["rel_pose"], model_output["gt_rel_pose"]
    for tag, fn in (("rot_distance", lambda t: t.mean()), ("rot_distance_degrees_mean", lambda t: (t / np.pi * 180).mean()),
                    ("rot_distance_degrees_std", lambda t: (t / np.pi * 180).std()), ("rot_distance_degrees_max", lambda t: (t / np.pi * 180).max())):
        m = torch.bmm(rel[:, :3, :3], gt_rel[:, :3, :3].transpose(1, 2))              # recomputed per scalar, as upstream
        writer.add_scalar(tag, fn(torch.acos(((m[:, 0, 0] + m[:, 1, 1] + m[:, 2, 2] - 1) / 2).clamp(-1, 1))), step)
    writer.add_scalar("tran_L1", F.mse_loss(rel[:, :3, 3], gt_rel[:, :3, 3]), step)
    writer.add_scalar("trgt_min", query.min(), step)
    writer.add_scalar("trgt_max", query.max(), step)


def synthetic_batch(dev):
    """A batch of two pairs without a model: the shapes of `forward(val=True)` at 65 536 rays x 128 samples."""
    inp = syn.make_inputs(2, S, S, 0, seed=900, full_image=True)
    flow = (syn.normal((2, 2, S // 4, S // 4), 901, std=2.0, stream=20), syn.normal((2, 2, S // 4, S // 4), 901, std=2.0, stream=21))
    rel = torch.eye(4).repeat(2, 1, 1)
    rel[:, :3, :3] = torch.from_numpy(syn._rot_y(-0.1).astype(np.float32))
    rel[:, 0, 3] = 0.3
    w = syn.uniform((4, 1024, 128), 902, 0.0, 1.0).repeat(1, S * S // 1024, 1)
    out = {"rgb": syn.uniform((2, 1, S * S, 3), 903, -1.2, 1.2), "depth_ray": syn.uniform((2, S * S, 1), 904, 0.0, 10.0),
           "at_wt": w / w.sum(-1, keepdim=True), "flow": flow, "rel_pose": rel,
           "gt_rel_pose": torch.eye(4).repeat(2, 1, 1)}
    mv = lambda o: {k: mv(v) for k, v in o.items()} if isinstance(o, dict) else (
        type(o)(mv(v) for v in o) if isinstance(o, (list, tuple)) else (o.to(dev) if torch.is_tensor(o) else o))
    return mv(inp), mv(out)


def log_forms(dev):
    inp, out = synthetic_batch(dev)
    table = jet_table()
    log, writer = SummaryLog(DroppingWriter(), lag=1), DroppingWriter()
    return {"hip": lambda: log.add(inp, out, 0, image_shape=(S, S)),
            "reference_style": lambda: reference_style(inp, out, writer, 0, table)}, log


def time_form(fn, iters, after=None):
    """(HIP-event ms per call, wall ms per call) of `iters` back-to-back calls."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    start.record()
    for _ in range(iters):
        fn()
    if after is not None:
        after()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters, (time.perf_counter() - t0) * 1e3 / iters


def traced_launches(form, calls=(2, 12)):
    """Launches per call of one form from two `rocprofv3 --kernel-trace` runs of this script (fresh processes)."""
    if shutil.which("rocprofv3") is None:
        return {"error": "rocprofv3 is not on PATH"}
    traces = []
    for k in calls:
        with tempfile.TemporaryDirectory() as d:
            cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "t", "--",
                   sys.executable, os.path.abspath(__file__), "--trace-form", form, "--trace-calls", str(k)]
            r = subprocess.run(cmd, cwd=d, capture_output=True, text=True, timeout=300)
            found = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
            if r.returncode or not found:
                return {"error": f"rocprofv3 run of {k} calls: exit {r.returncode}, {len(found)} trace files", "stderr": r.stderr[-400:]}
            with open(found[0], newline="") as f:
                traces.append([row["Kernel_Name"] for row in csv.DictReader(f)])
    per_call = (len(traces[1]) - len(traces[0])) / (calls[1] - calls[0])
    ours = sorted({n for n in traces[1] if any(k in n for k in ("flow_panels", "depth_jet", "attention_entropy"))})
    return {"kernels": per_call, "trace_rows": [len(t) for t in traces], "calls": list(calls), "hip_kernels_of_this_library": [n[:80] for n in ours]}


def spread(v):
    return {"runs": [round(x, 4) for x in v], "median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default="")
    ap.add_argument("--trace-form", choices=("hip", "reference_style"), help="only --trace-calls calls of one form (under rocprofv3)")
    ap.add_argument("--trace-calls", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.trace_form:
        forms, log = log_forms(dev)
        for _ in range(a.trace_calls):
            forms[a.trace_form]()
        log.flush()
        torch.cuda.synchronize()
        return

    # ---- (c) launches of one call, traced in fresh processes before this one opens the device
    traced = {name: traced_launches(name) for name in ("hip", "reference_style")}
    assert torch.cuda.is_available(), "summaries_time.py measures on a HIP device"
    res = {"device": torch.cuda.get_device_name(0), "batch": "2 pairs of 256 x 256, at_wt (4, 65536, 128)", "iters": a.iters,
           "rounds": a.rounds, "c_launches_per_call_rocprofv3_kernel_trace": traced}

    # ---- (a) the two forms of the log on the same batch
    forms, log = log_forms(dev)
    for name, fn in forms.items():
        time_form(fn, 5, log.flush if name == "hip" else None)
    ev = {k: [] for k in forms}
    wall = {k: [] for k in forms}
    for _ in range(a.rounds):
        for name, fn in forms.items():
            e, w = time_form(fn, a.iters, log.flush if name == "hip" else None)
            ev[name].append(e)
            wall[name].append(w)
    res["a_log_ms_per_batch"] = {k: {"hip_events": spread(ev[k]), "wall_back_to_back": spread(wall[k])} for k in ev}
    res["a_note"] = ("back-to-back calls on one batch; `hip` is SummaryLog(lag=1).add, the copy and the write of the entry before "
                     "it included, and a flush at the end of each window; where the host enqueues slower than the device runs, "
                     "both clocks show the host's enqueue rate, not kernel time")

    # ---- (b) the render loop
    model = CoPoNeRF.CoPoNeRF(n_view=2)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(syn.make_full_weights(shapes), strict=True)
    model = model.to(dev).eval()
    mv = lambda o: {k: mv(v) for k, v in o.items()} if isinstance(o, dict) else (o.to(dev) if torch.is_tensor(o) else o)
    batches = [mv(syn.make_inputs(2, S, S, 0, seed=700 + i, full_image=True)) for i in range(a.pairs)]
    table = jet_table()

    def loop(form):
        writer = DroppingWriter()
        slog = SummaryLog(writer, lag=1)
        with torch.no_grad():
            for step, (inp, out) in enumerate(render_images(model, batches)):
                if form == "summary_log":
                    slog.add(inp, out, step, image_shape=(S, S))
                elif form == "reference_style":
                    reference_style(inp, out, writer, step, table)
        slog.flush()
        torch.cuda.synchronize()

    loops = ["render_only", "summary_log", "reference_style"]
    for f in loops:
        loop(f)
    times = {f: [] for f in loops}
    for _ in range(a.rounds):
        for f in loops:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loop(f)
            times[f].append((time.perf_counter() - t0) * 1e3 / a.pairs)
    res["b_render_loop_ms_per_batch_of_2"] = {f: spread(times[f]) for f in loops}
    res["b_note"] = f"{a.pairs} batches of two 256 x 256 images per loop, wall clock around a final synchronise; summary_log includes its flush"
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
