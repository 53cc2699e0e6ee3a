"""What the on-device evaluation metrics cost (coponerf_amd/evaluate.py), on one MI355X.

  (a) `image_metrics` (csrc/image_metrics.hip) for 2 x 256 x 256 images against the stock-op composition of the same
      arithmetic - clamp and rescale, reflect pad, five depthwise 11 x 11 `conv2d` calls, the elementwise quotient, crop,
      means - alternating in one process, by HIP events and by wall clock around a synchronise;
  (b) the per-pair wall time of `pipeline.render_images` + `Evaluator.add` over `--pairs` batches of two 256 x 256 images,
      against the same loop with the reference's per-pair host reads (five `.item()` and two image copies to numpy,
      test.py:246-266), and - where scipy is installed - with its SSIM filter on the CPU as well;
  (c) kernel launches of one call of both metric forms: this script runs itself with `--trace-form` under
      `rocprofv3 --kernel-trace` for 2 and for 12 calls of a form and divides the difference of the traces' rows by 10
      (one-off kernels - building the inputs - cancel); torch.profiler's device events of one call are recorded beside it.

    python tools/eval_time.py [--pairs 8] [--rounds 5] [--iters 200] [--out profiles/r09_eval_metrics.json]
"""
import argparse
import json
import os
import csv
import glob
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
from coponerf_amd.evaluate import Evaluator, image_metrics, pose_metrics    # noqa: E402
from coponerf_amd.pipeline import render_images                         # noqa: E402


def stock_image_metrics(pred, target, window2d):
    """The arithmetic of image_metrics as stock device ops; (N, 3) like it.  The crop makes the padding mode immaterial."""
    p = (pred.clamp(-1, 1) + 1) * 0.5
    t = (target + 1) * 0.5
    mse = ((p - t) ** 2).mean(dim=(1, 2, 3))
    psnr = -10.0 * torch.log(mse) / np.log(10.0)
    x, y = p.permute(0, 3, 1, 2), t.permute(0, 3, 1, 2)
    blur = lambda v: F.conv2d(F.pad(v, (5, 5, 5, 5), mode="reflect"), window2d, groups=3)
    ux, uy, uxx, uyy, uxy = blur(x), blur(y), blur(x * x), blur(y * y), blur(x * y)
    vx, vy, vxy = uxx - ux * ux, uyy - uy * uy, uxy - ux * uy
    s = ((2 * ux * uy + 1e-4) * (2 * vxy + 9e-4)) / ((ux * ux + uy * uy + 1e-4) * (vx + vy + 9e-4))
    ssim = s[:, :, 5:-5, 5:-5].mean(dim=(1, 2, 3))
    return torch.stack((mse, psnr, ssim), dim=-1)


def window2d(dev):
    x = torch.arange(-5, 6, dtype=torch.float64)
    g = torch.exp(-x * x / (2 * 1.5 * 1.5))
    g = g / g.sum()
    return (g[:, None] * g[None, :]).float().expand(3, 1, 11, 11).contiguous().to(dev)


def time_form(fn, iters):
    """(HIP-event ms per call, wall ms per call) of `iters` back-to-back calls."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters, (time.perf_counter() - t0) * 1e3 / iters


def metric_forms(dev):
    """The two forms of (a) and (c) on the same 2 x 256 x 256 images."""
    pred = (syn.uniform((2, 256, 256, 3), 11, -1.2, 1.2)).to(dev)
    target = (pred * 0.9 + syn.normal((2, 256, 256, 3), 12, 0.05).to(dev)).contiguous()
    w2 = window2d(dev)
    return {"hip": lambda: image_metrics(pred, target), "stock": lambda: stock_image_metrics(pred, target, w2)}


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
    names = sorted({n for n in traces[1] if traces[1].count(n) > traces[0].count(n)})
    return {"kernels": per_call, "trace_rows": [len(t) for t in traces], "calls": list(calls), "names": [n[:80] for n in names]}


def launches(fn):
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == DeviceType.CUDA and not e.name.lower().startswith(("memcpy", "memset"))]
    return len(names), sorted(set(names))


def spread(v):
    return {"runs": [round(x, 4) for x in v], "median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def host_metric_block(out, gt, H, W, cpu_ssim):
    """test.py:222-269 as the reference runs it: device ops, five .item() reads, both images to numpy (and, with scipy, the
    SSIM filter on the CPU).  Returns the numbers so that nothing is optimised away."""
    B = out["rel_pose"].shape[0]
    rgb = ((out["rgb"].view(B, H, W, 3).clamp(-1, 1) + 1) * 0.5)
    target = (gt.view(B, H, W, 3) + 1) * 0.5
    pose = pose_metrics(out["rel_pose"], out["gt_rel_pose"])
    psnr_of = lambda m: -10.0 * torch.log(m) / np.log(10.0)
    mse = ((rgb - target) ** 2).mean()
    per = [((rgb[b] - target[b]) ** 2).mean() for b in range(B)]
    vals = [mse.item(), psnr_of(mse).item()] + [m.item() for m in per] + [psnr_of(per[0]).item()]     # five reads
    rgb_np, target_np = rgb.cpu().numpy(), target.cpu().numpy()
    if cpu_ssim:
        from scipy.ndimage import gaussian_filter
        for b in range(B):
            for c in range(3):
                x, y = rgb_np[b, ..., c], target_np[b, ..., c]
                f = lambda v: gaussian_filter(v, sigma=1.5, truncate=3.5, mode="reflect")
                ux, uy, uxx, uyy, uxy = f(x), f(y), f(x * x), f(y * y), f(x * y)
                s = ((2 * ux * uy + 1e-4) * (2 * (uxy - ux * uy) + 9e-4)) / ((ux * ux + uy * uy + 1e-4) * (uxx - ux * ux + uyy - uy * uy + 9e-4))
                vals.append(float(s[5:-5, 5:-5].mean(dtype=np.float64)))
    return vals, pose


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default="")
    ap.add_argument("--trace-form", choices=("hip", "stock"), help="only --trace-calls calls of one form (under rocprofv3)")
    ap.add_argument("--trace-calls", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.trace_form:
        fn = metric_forms(dev)[a.trace_form]
        for _ in range(a.trace_calls):
            fn()
        torch.cuda.synchronize()
        return

    # ---- (c) launches of one call, traced in fresh processes before this one opens the device
    traced = {name: traced_launches(name) for name in ("hip", "stock")}
    assert torch.cuda.is_available(), "eval_time.py measures on a HIP device"
    res = {"device": torch.cuda.get_device_name(0), "shape": [2, 256, 256, 3], "iters": a.iters, "rounds": a.rounds}

    # ---- (a) the two metric forms on the same images
    forms = metric_forms(dev)
    hip, stock = forms["hip"], forms["stock"]
    d = (hip() - stock()).abs().max(dim=0).values.tolist()
    res["hip_vs_stock_max_abs_diff"] = dict(zip(("mse", "psnr", "ssim"), d))
    for fn in (hip, stock):
        time_form(fn, 20)
    ev = {"hip": [], "stock": []}
    wall = {"hip": [], "stock": []}
    for _ in range(a.rounds):
        for name, fn in (("hip", hip), ("stock", stock)):
            e, w = time_form(fn, a.iters)
            ev[name].append(e)
            wall[name].append(w)
    res["a_image_metrics_ms_per_call"] = {k: {"hip_events": spread(ev[k]), "wall_back_to_back": spread(wall[k])} for k in ev}
    res["a_note"] = ("back-to-back calls: where the host enqueues slower than the device runs, both clocks show the host's enqueue "
                     "rate, not kernel time")

    res["c_launches_per_call"] = {}
    for name, fn in (("hip", hip), ("stock", stock)):
        n, _ = launches(fn)
        res["c_launches_per_call"][name] = {"rocprofv3_kernel_trace": traced[name], "torch_profiler_device_events": n}

    # ---- (b) the evaluation loop
    model = CoPoNeRF.CoPoNeRF(n_view=2)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    model.load_state_dict(syn.make_full_weights(shapes), strict=True)
    model = model.to(dev).eval()
    mv = lambda o: {k: mv(v) for k, v in o.items()} if isinstance(o, dict) else (o.to(dev) if torch.is_tensor(o) else o)
    batches = [mv(syn.make_inputs(2, 256, 256, 0, seed=700 + i, full_image=True)) for i in range(a.pairs)]
    try:
        import scipy.ndimage  # noqa: F401
        have_scipy = True
    except ImportError:
        have_scipy = False

    def loop(form):
        sink = []
        evl = Evaluator()
        with torch.no_grad():
            for inp, out in render_images(model, batches):
                gt = inp["query"]["rgb"]
                if form == "render_only":
                    continue
                if form == "device":
                    evl.add(out, gt, [0.6, 0.8])
                else:
                    sink.append(host_metric_block(out, gt, 256, 256, form == "host_reads_cpu_ssim"))
        if form == "device":
            sink.append(evl.summary())                      # the one read, inside the timed window
        torch.cuda.synchronize()
        return sink

    forms = ["render_only", "device", "host_reads"] + (["host_reads_cpu_ssim"] if have_scipy else [])
    for f in forms:
        loop(f)
    times = {f: [] for f in forms}
    for _ in range(a.rounds):
        for f in forms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loop(f)
            times[f].append((time.perf_counter() - t0) * 1e3 / a.pairs)
    res["b_eval_loop_ms_per_batch_of_2"] = {f: spread(times[f]) for f in forms}
    res["b_note"] = (f"{a.pairs} batches of two 256 x 256 images per loop, wall clock around a final synchronise; `device` includes "
                     "summary()'s one read; host_reads_cpu_ssim " + ("uses scipy.ndimage.gaussian_filter" if have_scipy else "not measured: scipy is not installed"))
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
