"""What the LPIPS training term costs (losses.LossConfig.lpips), on one MI355X, in one process, on
LPIPS.synthetic weights.  Every traced child runs before this process opens the device; one that fails ends the script.

  (a) the term alone: `LPIPS.differentiable` forward + backward on four 32 x 32 patches against a stock-op composition of the
      same network under autograd (the clamp, the round trip, the scaling layer, thirteen library convolutions in NCHW, the head
      as torch ops - `StockLPIPS` below), alternating, by HIP events and by wall clock around a synchronise; launches per call
      of each form from a `rocprofv3 --kernel-trace` run of this script (the rows between two marker kernels, after warm-up calls).
  (b) the BASELINE configs[2] training step (4 pairs x 4 096 rays x 64 samples at 256 x 256, bench.py's batch and weights):
        plain        bench.py's step as it is, without the term - the step of the commit before
        patch_rays   the same without the term, pairs 0 and 1 with the rays of a 64 x 64 window (the loader's mask [1, 1, 0, 0])
        hip          patch_rays with the term through csrc/lpips.hip
        stock        patch_rays with the term through the stock composition
      alternating, wall clock around a synchronise per window; launches per step of each from kernel traces.
      4 096 rays make a 64 x 64 patch (BatchAssembler(rays=4096, lpips=True, patch=64)); the reference's own 32 x 32 patches go
      with its 1 024 rays.

    python tools/lpips_loss_time.py [--rounds 5] [--iters 30] [--steps 10] [--out profiles/r14_lpips_loss.json]
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from summaries_time import spread, time_form                                          # noqa: E402
from coponerf_amd import CoPoNeRF, _hip, lpips as cl, synthetic as syn                # noqa: E402
from coponerf_amd.losses import LossConfig                                             # noqa: E402
from coponerf_amd.train_step import TrainStep                                         # noqa: E402

SEED, WEIGHT = 3, 0.1
STEP_FORMS = ("plain", "patch_rays", "hip", "stock")


class StockLPIPS(torch.nn.Module):
    """The network of coponerf_amd.lpips.LPIPS as stock fp32 device ops under autograd, with its weights: no kernel of this
    package.  `differentiable(p, t)` like LPIPS's; the gradient flows to p only."""

    def __init__(self, lp: cl.LPIPS):
        super().__init__()
        self.lp = lp
        self.register_buffer("shift", torch.tensor([-0.030, -0.088, -0.188]).view(1, 3, 1, 1))
        self.register_buffer("scale", torch.tensor([0.458, 0.448, 0.450]).view(1, 3, 1, 1))

    def differentiable(self, p, t):
        lp, N = self.lp, p.shape[0]
        rt = lambda x: ((x + 1.0) * 0.5 - 0.5) * 2.0
        x = (torch.cat((rt(p.clamp(-1.0, 1.0)), rt(t.detach()))) - self.shift) / self.scale
        total = 0
        for j, block in enumerate(cl.BLOCKS):
            if j:
                x = F.max_pool2d(x, 2, 2)
            for i in block:
                w, b = (lp.stem_weight, lp.stem_bias) if i == 0 else (getattr(lp, f"w{i}"), getattr(lp, f"b{i}"))
                x = F.relu(F.conv2d(x, w, b, padding=1))
            a = x / (x.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
            d = (a[:N] - a[N:].detach()).pow(2)
            total = total + (d * getattr(lp, f"lin{j}").view(1, -1, 1, 1)).sum(1, keepdim=True).mean(dim=(2, 3)).view(N)
        return total


def patches(dev, n=4, side=32):
    t = syn.uniform((n, 3, side, side), 21, -1.0, 1.0, stream=1).float()
    p = (0.9 * t + syn.normal((n, 3, side, side), 21, 0.15, stream=2)).float()
    return p.to(dev), t.to(dev)


def term_forms(dev):
    lp = cl.LPIPS.synthetic(SEED).to(dev)
    nets = {"hip": lp, "stock": StockLPIPS(lp).to(dev)}
    p, t = patches(dev)
    p.requires_grad_(True)

    def run(net):
        p.grad = None
        net.differentiable(p, t).mean().backward()
    return {k: (lambda net=net: run(net)) for k, net in nets.items()}, p


def step_forms(dev, only=STEP_FORMS, pairs=4, rays=4096, samples=64):
    """bench.py's configs[2] batch and weights, one model and one TrainStep per form in `only` (the steps update their own copy)."""
    lp = cl.LPIPS.synthetic(SEED).to(dev)
    stock = StockLPIPS(lp).to(dev)
    mv = lambda o: o.to(dev) if torch.is_tensor(o) else {k: mv(v) for k, v in o.items()}
    plain = syn.make_inputs(pairs, 256, 256, rays, seed=61)
    windows = syn.make_inputs(pairs, 256, 256, rays, seed=61)
    side = int(round(rays ** 0.5))
    assert side * side == rays
    ys, xs = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    for b, (x0, y0) in enumerate(((40, 100), (150, 20))):
        windows["query"]["uv"][b, 0] = torch.from_numpy(np.stack((x0 + xs.reshape(-1), y0 + ys.reshape(-1)), -1).astype(np.float32))
    mask = torch.tensor([1, 1] + [0] * (pairs - 2), dtype=torch.int64)
    plain, windows = mv(plain), mv(windows)
    windows["query"]["mask"] = mask                                                    # on the host
    forms = {}
    for name in only:
        model = CoPoNeRF.CoPoNeRF(n_view=2, npoints=samples)
        shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
        model.load_state_dict(syn.make_full_weights(shapes, seed=11), strict=True)
        model = model.to(dev).train()
        inp = plain if name == "plain" else windows
        if name in ("plain", "patch_rays"):
            step = TrainStep(model)
        else:
            step = TrainStep(model, loss=LossConfig(lpips=WEIGHT), perceptual=lp if name == "hip" else stock)
        forms[name] = (lambda step=step, inp=inp: step(inp, inp["query"]["rgb"]))
    return forms


def trace_rows(argv, timeout):
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "t", "--", sys.executable, os.path.abspath(__file__)] + argv
        r = subprocess.run(cmd, cwd=d, capture_output=True, text=True, timeout=timeout)
        found = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if r.returncode or not found:
            return {"error": f"rocprofv3 run of {argv}: exit {r.returncode}, {len(found)} trace files", "stderr": r.stderr[-400:]}
        with open(found[0], newline="") as f:
            return list(csv.DictReader(f))


MARKER = "depth_jet_kernel"                                # a kernel of this package that none of the forms launches


def marker(dev):
    """One launch of cpn_depth_jet on the current stream: the trace's rows between two of them are the timed calls'."""
    depth, table = torch.zeros(64, device=dev), torch.zeros(256, 3, device=dev)
    out = torch.empty(64, 3, device=dev)
    torch.cuda.synchronize()
    _hip.call("cpn_depth_jet", depth.data_ptr(), 64, table.data_ptr(), out.data_ptr(), _hip.stream_handle())
    torch.cuda.synchronize()


def traced(kind, forms, warm, calls, timeout):
    """Launches per call of each form from one kernel trace of a fresh process: `warm` calls (the libraries choose their
    algorithms there, with launches of their own), a marker kernel, `calls` calls, a marker kernel; the rows between the markers."""
    if shutil.which("rocprofv3") is None:
        return {"error": "rocprofv3 is not on PATH"}
    out = {"warm_up_calls": warm, "calls": calls}
    for name in forms:
        rows = trace_rows([f"--trace-{kind}", name, "--trace-warm", str(warm), "--trace-calls", str(calls)], timeout)
        if isinstance(rows, dict):
            return rows
        rows.sort(key=lambda r: int(r["Start_Timestamp"]))
        marks = [i for i, r in enumerate(rows) if MARKER in r["Kernel_Name"]]
        if len(marks) != 2:
            return {"error": f"{len(marks)} marker launches in the trace of {kind} {name}"}
        mine = rows[marks[0] + 1:marks[1]]
        out[name] = {"launches_per_call": len(mine) / calls,
                     "of_csrc_lpips_per_call": sum("lpips_" in r["Kernel_Name"] for r in mine) / calls}
        print(f"traced {calls} calls of {kind} {name}: {out[name]}", file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30, help="calls of the term per window")
    ap.add_argument("--steps", type=int, default=10, help="training steps per window")
    ap.add_argument("--out", default="")
    ap.add_argument("--trace-term", choices=("hip", "stock"), help="only --trace-calls calls of one form of the term (under rocprofv3)")
    ap.add_argument("--trace-step", choices=STEP_FORMS, help="only --trace-calls steps of one form (under rocprofv3)")
    ap.add_argument("--trace-calls", type=int, default=2)
    ap.add_argument("--trace-warm", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.trace_term or a.trace_step:
        fn = term_forms(dev)[0][a.trace_term] if a.trace_term else step_forms(dev, (a.trace_step,))[a.trace_step]
        for _ in range(a.trace_warm):
            fn()
        marker(dev)
        for _ in range(a.trace_calls):
            fn()
        marker(dev)
        return

    # ---- launches, traced in fresh processes before this one opens the device
    launches_term = traced("term", ("hip", "stock"), 3, 10, 300)
    if "error" in launches_term:                            # a child that failed may have faulted the device: start nothing more on it
        sys.exit(f"lpips_loss_time.py: {launches_term}")
    launches_step = traced("step", STEP_FORMS[1:], 3, 3, 400)          # `plain` launches what `patch_rays` does
    if "error" in launches_step:
        sys.exit(f"lpips_loss_time.py: {launches_step}")
    assert torch.cuda.is_available(), "lpips_loss_time.py measures on a HIP device"

    # ---- (a) the term alone
    forms, p = term_forms(dev)
    grads = {}
    for k, fn in forms.items():
        time_form(fn, 5)
        grads[k] = p.grad.clone()
    agree = float((grads["hip"] - grads["stock"]).abs().max() / grads["stock"].abs().max())
    ev, wall = {k: [] for k in forms}, {k: [] for k in forms}
    for _ in range(a.rounds):
        for k, fn in forms.items():
            e, w = time_form(fn, a.iters)
            ev[k].append(e)
            wall[k].append(w)
    term = {k: {"hip_events_ms": spread(ev[k]), "wall_back_to_back_ms": spread(wall[k])} for k in forms}
    del forms, p, grads
    torch.cuda.empty_cache()

    # ---- (b) the training step
    steps = step_forms(dev)
    info = {}
    for k, fn in steps.items():
        for _ in range(3):
            info[k] = fn()
    torch.cuda.synchronize()
    losses = {k: {n: float(v) for n, v in r["losses"].items()} for k, r in info.items()}
    stepped = {k: bool(r["stepped"]) for k, r in info.items()}
    ms = {k: [] for k in steps}
    for _ in range(a.rounds):
        for k, fn in steps.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / a.steps)
            print(f"{k}: {ms[k][-1]:.2f} ms per step", file=sys.stderr, flush=True)
    res = {"device": torch.cuda.get_device_name(0), "weights": f"LPIPS.synthetic({SEED}); no real VGG weights ship", "rounds": a.rounds,
           "term_alone": {"batch": "4 patches of 32 x 32, forward + backward of the mean", "iters": a.iters,
                          "forward_backward": term, "launches_rocprofv3_kernel_trace": launches_term,
                          "max_grad_difference_hip_vs_stock_relative": agree},
           "training_step": {"batch": "configs[2]: 4 pairs x 4096 rays x 64 samples, 256 x 256, bench.py's inputs (seed 61) and weights (seed 11)",
                             "patch_pairs": "pairs 0 and 1: the rays of a 64 x 64 window; mask [1, 1, 0, 0]", "weight": WEIGHT,
                             "steps_per_window": a.steps, "ms_per_step_wall": {k: spread(v) for k, v in ms.items()},
                             "launches_rocprofv3_kernel_trace": launches_step, "losses_after_warm_up": losses, "stepped": stepped},
           "note": ("forms alternate inside every round; `plain` is bench.py's training step (TrainStep(model) on its batch), `patch_rays` "
                    "the same step on the batch the two forms with the term see; a step's time is the host clock around a window that "
                    "ends in a synchronise; the traces are runs of their own, fresh processes, taken first")}
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
