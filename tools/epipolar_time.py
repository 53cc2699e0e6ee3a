"""What the log's two drawings cost (coponerf_amd/summaries.py: epipolar=True, contour=True), on one MI355X,
for a batch of two 256 x 256 pairs (tools/summaries_time.synthetic_batch with a true pose that has a translation, so that
every line of both kinds is drawn; the script checks that and says how many were).  A traced child that fails ends the script
before it opens the device itself.

  (a) `SummaryLog(lag=1).add` with both switches on against the same call with them off, alternating in one process, by HIP
      events and by wall clock around a synchronise.
  (b) the three kernels of csrc/epipolar.hip: this script runs itself with `--trace-calls` under `rocprofv3 --kernel-trace`
      for 2 and for 12 calls of the log with both switches on; launches per call from the difference of the traces' rows
      (one-off kernels cancel), kernel times from the trace's own time stamps.

There is no host-side OpenCV form to compare with: `cv2` is not installed where this was written.

    python tools/epipolar_time.py [--rounds 5] [--iters 50] [--out profiles/r13_epipolar.json]
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

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from summaries_time import DroppingWriter, S, spread, synthetic_batch, time_form     # noqa: E402
from coponerf_amd import synthetic as syn                                             # noqa: E402
from coponerf_amd.summaries import SummaryLog, default_points, epipolar_lines         # noqa: E402

KERNELS = ("epipolar_lines_kernel", "epipolar_panels_kernel", "mask_contour_kernel")


def traced(calls=(2, 12)):
    if shutil.which("rocprofv3") is None:
        return {"error": "rocprofv3 is not on PATH"}
    rows = []
    for k in calls:
        with tempfile.TemporaryDirectory() as d:
            cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "t", "--",
                   sys.executable, os.path.abspath(__file__), "--trace-calls", str(k)]
            r = subprocess.run(cmd, cwd=d, capture_output=True, text=True, timeout=300)
            found = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
            if r.returncode or not found:
                return {"error": f"rocprofv3 run of {k} calls: exit {r.returncode}, {len(found)} trace files", "stderr": r.stderr[-400:]}
            with open(found[0], newline="") as f:
                rows.append(list(csv.DictReader(f)))
    span = calls[1] - calls[0]
    out = {"calls": list(calls), "trace_rows": [len(r) for r in rows], "launches_per_call_all_kernels": (len(rows[1]) - len(rows[0])) / span}
    for name in KERNELS:
        mine = [[r for r in t if name in r["Kernel_Name"]] for t in rows]
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in mine[1][2:]]          # the first calls warm up
        out[name] = {"launches_per_call": (len(mine[1]) - len(mine[0])) / span,
                     "us": {"median": round(statistics.median(us), 2), "min": round(min(us), 2), "max": round(max(us), 2), "n": len(us)}}
    return out


def batch(dev):
    """summaries_time.synthetic_batch with a true pose that has a translation: under its identity gt_rel_pose F_gt is 0, every
    GT line has b == 0 and is skipped, and the panels kernel would be timed on half of its lines."""
    inp, out = synthetic_batch(dev)
    out = dict(out)
    gt = torch.eye(4).repeat(2, 1, 1)
    gt[:, :3, :3] = torch.from_numpy(syn._rot_y(-0.12).astype(np.float32))
    gt[:, :3, 3] = torch.tensor([0.3, 0.02, 0.0])
    out["gt_rel_pose"] = gt.to(dev)
    return inp, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default="")
    ap.add_argument("--trace-calls", type=int, default=0, help="only that many calls of the log with both switches on (under rocprofv3)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.trace_calls:
        inp, out = batch(dev)
        log = SummaryLog(DroppingWriter(), lag=1, epipolar=True, contour=True)
        for _ in range(a.trace_calls):
            log.add(inp, out, 0, image_shape=(S, S))
        log.flush()
        torch.cuda.synchronize()
        return

    kernels = traced()                                      # fresh processes, before this one opens the device
    if "error" in kernels:                                  # a child that failed may have faulted the device: start nothing more on it
        sys.exit(f"epipolar_time.py: {kernels}")
    assert torch.cuda.is_available(), "epipolar_time.py measures on a HIP device"
    inp, out = batch(dev)
    points = torch.tensor(default_points(S), dtype=torch.int32).to(dev)
    valid = epipolar_lines(inp["context"]["intrinsics"].contiguous(), out["rel_pose"], out["gt_rel_pose"], points, S)[3]
    drawn = [int(v) for v in valid.sum(dim=(1, 2)).tolist()]
    assert drawn == [2 * len(points)] * 2, f"the timing batch skips lines: {drawn}"
    logs = {"off": SummaryLog(DroppingWriter(), lag=1), "on": SummaryLog(DroppingWriter(), lag=1, epipolar=True, contour=True)}
    forms = {k: (lambda log=log: log.add(inp, out, 0, image_shape=(S, S))) for k, log in logs.items()}
    for k, fn in forms.items():
        time_form(fn, 5, logs[k].flush)
    ev, wall = {k: [] for k in forms}, {k: [] for k in forms}
    for _ in range(a.rounds):
        for k, fn in forms.items():
            e, w = time_form(fn, a.iters, logs[k].flush)
            ev[k].append(e)
            wall[k].append(w)
    res = {"device": torch.cuda.get_device_name(0), "batch": "2 pairs of 256 x 256, at_wt (4, 65536, 128)", "iters": a.iters,
           "rounds": a.rounds, "lines_drawn_pred_gt": drawn, "kernels_rocprofv3_kernel_trace": kernels,
           "log_add_ms_per_batch": {k: {"hip_events": spread(ev[k]), "wall_back_to_back": spread(wall[k])} for k in forms},
           "note": ("the batch of tools/summaries_time.py with a true pose that has a translation, so that all 2 x 2 x 9 lines are drawn; "
                    "`off` is SummaryLog(lag=1).add as before, `on` the same with epipolar=True, contour=True (ten images instead of "
                    "eight), alternating on one batch, the copy and the write of the entry before included; where the host enqueues "
                    "slower than the device runs, both clocks show the host's enqueue rate.  No OpenCV form was available to compare with.")}
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
