"""Times the evaluation metrics: the HIP path (omnidata_amd.gpu_metrics) against omnidata_amd.metrics, torch ops on the same
CUDA tensors, which is how the metrics were computed before.

    python tools/metrics_bench.py [--sizes 1,32] [--hw 384] [--iters 20] [--repeats 7] [--min-window-ms 50] [--json out.json]

Inputs are generated on the device from a seed: for normals targets 0.5 n + 0.5 for random unit n and the prediction the
target plus noise, for depth a target in [0.05, 0.95] and the prediction the target plus noise, an 80 % mask.  Four
measurements per task and batch size, all ending on the host as the reference's callers need them.  Each is the median of
`repeats` windows between HIP events, with the smallest and the largest window next to it; a window holds at least `iters`
calls and at least 50 ms of work, and the windows of the two paths alternate:
  batch row    gpu_metrics.get_metrics (one launch sequence, one copy of the row)       against metrics.get_metrics
  image rows   gpu_metrics.<task>_metrics(per_image=True) and one copy of the [B, fields] rows
                                                                                          against B calls of metrics.get_metrics
Also prints the time of the launch sequence alone (no copy; a synchronise ends the window), the bytes per second it
achieves on what the algorithm has to move -- normal: 25 B per pixel read, the 8-byte key written and read in 7 select
passes, 89 B per pixel; depth: 9 B per pixel -- and the largest difference between the two paths by the criterion
|d| / max(1, |v|) of the tests.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BYTES_PER_PIXEL = {"normal": 25 + 8 + 7 * 8, "depth_zbuffer": 9}


def inputs(task, B, hw, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    if task == "normal":
        n = torch.randn(B, 3, hw, hw, generator=g, device="cuda")
        t = 0.5 * n / n.norm(dim=1, keepdim=True) + 0.5
        p = t + 0.2 * torch.randn(B, 3, hw, hw, generator=g, device="cuda")
    else:
        t = torch.rand(B, 1, hw, hw, generator=g, device="cuda") * 0.9 + 0.05
        p = (t + 0.05 * torch.randn(B, 1, hw, hw, generator=g, device="cuda")).clamp(min=0.0)
    m = torch.rand(B, 1, hw, hw, generator=g, device="cuda") < 0.8
    return p.contiguous(), t.contiguous(), m


def window(fn, calls):
    """milliseconds per call over one window of `calls` calls between two HIP events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def measure(fns: dict, iters, repeats, min_window_ms):
    """Every function of `fns` after two warm-up calls: `repeats` windows each, the functions ALTERNATING window by window so
    that drift of the machine hits all of them alike; a window holds at least `iters` calls and at least min_window_ms of
    work (sized from a first window that is thrown away).  -> {name: dict(median, min, max in ms per call, calls per window)}"""
    calls = {}
    for name, fn in fns.items():
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        calls[name] = max(iters, int(min_window_ms / max(window(fn, iters), 1e-4)) + 1)
    got = {name: [] for name in fns}
    for _ in range(repeats):
        for name, fn in fns.items():
            got[name].append(window(fn, calls[name]))
    return {name: dict(median=statistics.median(v), min=min(v), max=max(v), calls=calls[name]) for name, v in got.items()}


def worst(got: dict, want: dict) -> float:
    d = 0.0
    for k, v in want.items():
        if got[k] != got[k] or v != v:
            d = max(d, 0.0 if (got[k] != got[k]) == (v != v) else float("inf"))
        else:
            d = max(d, abs(got[k] - v) / max(1.0, abs(v)))
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,32")
    ap.add_argument("--hw", type=int, default=384)
    ap.add_argument("--iters", type=int, default=20, help="calls per window, at least")
    ap.add_argument("--repeats", type=int, default=7, help="windows per measurement")
    ap.add_argument("--min-window-ms", type=float, default=50.0)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("metrics_bench needs an AMD GPU: a timing taken anywhere else says nothing")
    from omnidata_amd import gpu_metrics as gm
    from omnidata_amd import metrics as tm
    rows = []
    for task in ("normal", "depth_zbuffer"):
        per_image = gm.normal_metrics if task == "normal" else gm.depth_metrics
        fields = gm.NORMAL_FIELDS if task == "normal" else gm.DEPTH_FIELDS
        for B in [int(s) for s in args.sizes.split(",")]:
            p, t, m = inputs(task, B, args.hw, seed=B)

            def hip_batch():
                return gm.get_metrics(p, t, task, m)

            def torch_batch():
                return tm.get_metrics(p, t, task, m)

            def hip_images():
                return torch.stack([per_image(p, t, m, per_image=True)[k] for k in fields], 1).cpu()

            def torch_images():
                return [tm.get_metrics(p[i:i + 1], t[i:i + 1], task, m[i:i + 1]) for i in range(B)]

            def hip_launches():
                gm._rows(task, p, t, m, False)

            px = B * args.hw * args.hw
            t_ms = measure(dict(hip_batch=hip_batch, torch_batch=torch_batch, hip_images=hip_images, torch_images=torch_images,
                                hip_launches=hip_launches), args.iters, args.repeats, args.min_window_ms)
            r = dict(task=task, B=B, hw=args.hw, valid=int(m.sum()), repeats=args.repeats)
            for name, v in t_ms.items():   # the median of the windows is the figure, min and max its spread
                r[name + "_ms"], r[name + "_ms_min"], r[name + "_ms_max"], r[name + "_calls"] = v["median"], v["min"], v["max"], v["calls"]
            r["hip_launches_TBps"] = BYTES_PER_PIXEL[task] * px / (r["hip_launches_ms"] * 1e-3) / 1e12
            r["batch_speedup"] = r["torch_batch_ms"] / r["hip_batch_ms"]
            r["images_speedup"] = r["torch_images_ms"] / r["hip_images_ms"]
            r["batch_worst_diff"] = worst(hip_batch(), torch_batch())
            hi, ti = hip_images().tolist(), torch_images()
            r["images_worst_diff"] = max(worst(dict(zip(fields[1:], hi[i][1:])), ti[i]) for i in range(B))
            rows.append(r)
            print(json.dumps(r))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
