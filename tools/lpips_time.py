"""What the on-device LPIPS costs (coponerf_amd/lpips.py), on one MI355X.  Synthetic weights throughout.

  (a) `LPIPS.forward` for two 256 x 256 pairs, and its split into stem kernel / library trunk / head kernel by HIP events,
      against a stock-op composition of the same network written here (library convolutions in NCHW including conv1_1, the
      scaling and the distance head as torch ops) - the two alternate in one process, five rounds;
  (b) the trunk alone, from the stem's NHWC output, in the two memory formats the head could be fed from: channels_last
      convolutions (the tapped maps are the head's NHWC as they are), and NCHW convolutions with one copy of relu1_1 in and one
      channels-last copy of each of the five tapped maps out (the module's form).  Both, like (a), once with the library free
      to choose and once restricted to deterministic algorithms (`torch.backends.cudnn.deterministic`), which is the state
      `get_z` puts the process in for inference and therefore the state every evaluation loop runs in;
  (c) kernel launches of one call of both forms of (a): this script runs itself with `--trace-form` under
      `rocprofv3 --kernel-trace` (no counters) for 12 calls and counts the trace's rows between a once-per-call kernel of
      consecutive calls, after two warm calls;
  (d) the per-batch wall time of the evaluation loop of DESIGN.md §4.8 (`pipeline.render_images` + `Evaluator.add` +
      one `summary()`), with and without `extra={"lpips": ...}`.

    python tools/lpips_time.py [--pairs 8] [--rounds 5] [--iters 50] [--out profiles/r11_lpips.json]
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

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from coponerf_amd import synthetic as syn                               # noqa: E402
from coponerf_amd import lpips as cl                                    # noqa: E402

SEED = 3
SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)


def stock_lpips(p, t, weights, biases, lins):
    """LPIPS-VGG as stock fp32 device ops: p, t (N, 3, H, W).  Not the module under test."""
    shift = torch.tensor(SHIFT, device=p.device).view(1, 3, 1, 1)
    scale = torch.tensor(SCALE, device=p.device).view(1, 3, 1, 1)
    x = torch.cat((p.clamp(-1.0, 1.0), t))
    x = ((x + 1.0) * 0.5 - 0.5) * 2.0
    x = (x - shift) / scale
    N, total, n = p.shape[0], 0, 0
    for j, block in enumerate(cl.BLOCKS):
        if j:
            x = F.max_pool2d(x, 2, 2)
        for _ in block:
            x = F.relu(F.conv2d(x, weights[n], biases[n], padding=1))
            n += 1
        a = x / (x.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        d = (a[:N] - a[N:]).pow(2)
        total = total + (d * lins[j].view(1, -1, 1, 1)).sum(1, keepdim=True).mean(dim=(2, 3)).view(N)
    return total


def trunk_channels_last(x, weights, biases):
    """conv1_2 .. conv5_3 in channels_last memory from the stem's relu1_1 view (weights channels_last too); the tapped maps
    are NHWC as they are (one copy where the library hands back another layout).  Not the module's form."""
    taps, n = [], 1
    for j, block in enumerate(cl.BLOCKS):
        if j:
            x = F.max_pool2d(x, 2, 2)
        for i in block:
            if i == 0:
                continue
            x = F.relu_(F.conv2d(x, weights[n], biases[n], padding=1))
            n += 1
        taps.append(x.permute(0, 2, 3, 1).contiguous())
    return taps


def images(dev, N=2, H=256, W=256):
    """The hook's views: (N, H, W, 3) memory seen as (N, 3, H, W)."""
    pred = syn.uniform((N, H, W, 3), 11, -1.2, 1.2).to(dev)
    target = (pred * 0.9 + syn.normal((N, H, W, 3), 12, 0.05).to(dev)).contiguous()
    return pred.permute(0, 3, 1, 2), target.permute(0, 3, 1, 2)


def forms(dev):
    p, t = images(dev)
    lp = cl.LPIPS.synthetic(SEED).to(dev)
    weights, biases, lins = ([x.to(dev) for x in part] for part in cl.parse_state_dict(cl.synthetic_state_dict(SEED)))
    with torch.no_grad():
        pc, tc = p.contiguous(), t.contiguous()             # the stock form gets NCHW memory, copied once outside the timing
    return {"hip": lambda: lp(p, t), "stock": lambda: stock_lpips(pc, tc, weights, biases, lins)}, lp, (p, t), (weights, biases, lins)


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


def split_module(lp, p, t, iters):
    """HIP-event ms per call of the module's three parts, each timed over `iters` calls of that part alone."""
    N = p.shape[0]
    pn, tn = lp._channels_last(p), lp._channels_last(t)
    x = lp.stem(pn, tn)
    taps = lp.trunk(x)
    return {"stem": time_form(lambda: lp.stem(pn, tn), iters)[0], "trunk": time_form(lambda: lp.trunk(x), iters)[0],
            "head": time_form(lambda: lp.head(taps, N), iters)[0]}


MARKER = {"hip": "lpips_stem_kernel", "stock": "CatArrayBatchedCopy"}     # a kernel every call of the form launches exactly once


def traced_launches(form, calls=12, warm=2):
    """Launches per call of one form, counted in ONE `rocprofv3 --kernel-trace` run of this script (a fresh process, no
    counters): the trace's rows in start order, cut at a kernel every call launches exactly once.  Each count is the whole number
    of rows from one call's marker to the next call's; the first `warm` calls (where the library searches and loads
    its kernels) and the last (nothing closes it) are left out."""
    if shutil.which("rocprofv3") is None:
        return {"error": "rocprofv3 is not on PATH"}
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "t", "--",
               sys.executable, os.path.abspath(__file__), "--trace-form", form, "--trace-calls", str(calls)]
        r = subprocess.run(cmd, cwd=d, capture_output=True, text=True, timeout=300)
        if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
            # a fault, abort or hang of the traced child: nothing more is started on the device
            sys.exit(f"rocprofv3 run of {calls} calls of `{form}` ended with {r.returncode}; stopping.\n{r.stderr[-800:]}")
        found = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if r.returncode or not found:
            return {"error": f"rocprofv3 run of {calls} calls: exit {r.returncode}, {len(found)} trace files", "stderr": r.stderr[-400:]}
        with open(found[0], newline="") as f:
            rows = list(csv.DictReader(f))
    return count_per_call([(int(row.get("Start_Timestamp") or i), row["Kernel_Name"]) for i, row in enumerate(rows)], form, calls, warm)


def count_per_call(stamped, form, calls, warm):
    names = [n for _, n in sorted(stamped, key=lambda e: e[0])]
    marks = [i for i, n in enumerate(names) if MARKER[form] in n]
    if len(marks) != calls:
        return {"error": f"{len(marks)} `{MARKER[form]}` rows in a trace of {calls} calls", "trace_rows": len(names)}
    counts = [marks[i + 1] - marks[i] for i in range(warm, calls - 1)]
    steady = names[marks[warm]:marks[warm + 1]]
    per_name = {}
    for n in steady:                                        # shortened names can coincide: their counts add up
        per_name[n[:80]] = per_name.get(n[:80], 0) + 1
    return {"kernels": statistics.mode(counts), "per_call": counts, "trace_rows": len(names), "calls": calls, "warm": warm,
            "names": dict(sorted(per_name.items()))}


def spread(v):
    return {"runs": [round(x, 4) for x in v], "median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default="")
    ap.add_argument("--skip-loop", action="store_true", help="leave out (d), the evaluation loop")
    ap.add_argument("--trace-form", choices=("hip", "stock"), help="only --trace-calls calls of one form (under rocprofv3)")
    ap.add_argument("--trace-calls", type=int, default=12)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.trace_form:
        fn = forms(dev)[0][a.trace_form]
        with torch.no_grad():
            for _ in range(a.trace_calls):
                fn()
        torch.cuda.synchronize()
        return

    # ---- (c) launches of one call, traced in fresh processes before this one opens the device
    traced = {name: traced_launches(name) for name in ("hip", "stock")}
    assert torch.cuda.is_available(), "lpips_time.py measures on a HIP device"
    res = {"device": torch.cuda.get_device_name(0), "shape": [2, 3, 256, 256], "iters": a.iters, "rounds": a.rounds,
           "weights": f"LPIPS.synthetic({SEED}): no real VGG / lin weights were used for any number here"}
    res["c_launches_per_call"] = traced

    fs, lp, (p, t), (weights, biases, _) = forms(dev)
    w_cl = [None] + [w.contiguous(memory_format=torch.channels_last) for w in weights[1:]]

    def measure(deterministic):
        """(a) and (b) with the convolution library free (False) or restricted to deterministic algorithms (True)."""
        torch.backends.cudnn.deterministic = deterministic
        out = {}
        hip, stock = fs["hip"], fs["stock"]
        out["hip_vs_stock_abs_diff"] = (hip() - stock()).abs().tolist()
        out["values"] = hip().tolist()
        out["two_calls_bit_equal"] = {"hip": bool(torch.equal(hip(), hip())), "stock": bool(torch.equal(stock(), stock()))}
        for fn in (hip, stock):
            time_form(fn, 5)
        ev = {"hip": [], "stock": []}
        wall = {"hip": [], "stock": []}
        parts = {"stem": [], "trunk": [], "head": []}
        for _ in range(a.rounds):
            for name, fn in (("hip", hip), ("stock", stock)):
                e, w = time_form(fn, a.iters)
                ev[name].append(e)
                wall[name].append(w)
            for k, v in split_module(lp, p, t, a.iters).items():
                parts[k].append(v)
        out["a_lpips_ms_per_call"] = {k: {"hip_events": spread(ev[k]), "wall_back_to_back": spread(wall[k])} for k in ev}
        out["a_module_split_ms"] = {k: spread(v) for k, v in parts.items()}
        # ---- (b) the trunk's memory format, both from the stem's own output
        x = lp.stem(lp._channels_last(p), lp._channels_last(t))
        fmt = {"nchw_plus_copies": lambda: lp.trunk(x), "channels_last": lambda: trunk_channels_last(x, w_cl, biases)}
        iters = max(4, a.iters // 5)                        # the deterministic channels_last kernels take 0.3 s per trunk
        for fn in fmt.values():
            time_form(fn, 2)
        tf = {k: [] for k in fmt}
        for _ in range(a.rounds):
            for k, fn in fmt.items():
                tf[k].append(time_form(fn, iters)[0])
        out["b_trunk_format_ms"] = {k: spread(v) for k, v in tf.items()}
        out["b_iters"] = iters
        out["b_max_tap_diff"] = max(float((u - v).abs().max()) for u, v in zip(fmt["channels_last"](), fmt["nchw_plus_copies"]()))
        y = F.conv2d(x, w_cl[1], biases[1], padding=1)
        out["b_library_keeps_channels_last"] = bool(y.is_contiguous(memory_format=torch.channels_last) and not y.is_contiguous())
        return out

    with torch.no_grad():
        res["library_free"] = measure(False)
        res["library_deterministic"] = measure(True)
    res["a_note"] = ("back-to-back calls of two 256 x 256 pairs; the split times each part alone over the same number of calls, "
                     "so its three medians need not add up to the whole exactly.  library_deterministic is the state get_z "
                     "leaves the process in during inference, i.e. the state of (d)")
    torch.backends.cudnn.deterministic = False              # (d) starts from the process default; get_z sets its own state

    # ---- (d) the evaluation loop with and without the LPIPS column
    if not a.skip_loop:
        from coponerf_amd import CoPoNeRF
        from coponerf_amd.evaluate import Evaluator
        from coponerf_amd.pipeline import render_images
        model = CoPoNeRF.CoPoNeRF(n_view=2)
        shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
        model.load_state_dict(syn.make_full_weights(shapes), strict=True)
        model = model.to(dev).eval()
        mv = lambda o: {k: mv(v) for k, v in o.items()} if isinstance(o, dict) else (o.to(dev) if torch.is_tensor(o) else o)
        batches = [mv(syn.make_inputs(2, 256, 256, 0, seed=700 + i, full_image=True)) for i in range(a.pairs)]

        def loop(with_lpips):
            evl = Evaluator(extra={"lpips": lp} if with_lpips else None)
            with torch.no_grad():
                for inp, out in render_images(model, batches):
                    evl.add(out, inp["query"]["rgb"], [0.6, 0.8])
            s = evl.summary()                               # the one read, inside the timed window
            torch.cuda.synchronize()
            return s

        for f in (False, True):
            loop(f)
        times = {"device": [], "device_with_lpips": []}
        for _ in range(a.rounds):
            for key, f in (("device", False), ("device_with_lpips", True)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                loop(f)
                times[key].append((time.perf_counter() - t0) * 1e3 / a.pairs)
        res["d_eval_loop_ms_per_batch_of_2"] = {k: spread(v) for k, v in times.items()}
        res["d_note"] = f"{a.pairs} batches of two 256 x 256 images per loop, wall clock around a final synchronise, summary()'s one read included"
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
