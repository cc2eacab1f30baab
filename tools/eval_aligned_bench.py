"""Times scale-and-shift-aligned depth evaluation: the one call (dptx_eval_depth_aligned) against what it replaces.

    python tools/eval_aligned_bench.py [--sizes 1,32] [--hw 384] [--align lstsq] [--iters 20] [--repeats 7] [--json out.json]

Every path leaves the [B + 1, 15] rows (B images and the batch) on the device; a synchronise ends each window.  Medians of
alternating windows between HIP events, as tools/metrics_bench.py (its `measure`):
  one call      gpu_metrics.aligned_depth_metrics' launch sequence: statistics, solve, one metric pass, one finalize
  composition   the entry points that existed before it: dptx_midas_stats, torch mul / add / clamp that write and re-read a
                [B,1,H,W] temporary, dptx_eval_depth twice (per image, whole batch), torch ops for fields 8-14
  torch only    the same with torch ops for the fit and for every field
Inputs: a target in [0.1, 0.9], the prediction (t - 0.2) / 1.7 plus N(0, 0.02), an 80 % mask, generated on the device.
Also prints the largest difference of the two other paths from the one call by the criterion |d| / max(1, |v|) of the tests, and
the bytes the one call has to move: 9 B per pixel in each of the passes over the inputs (LSTSQ: count, sums, metrics = 3;
MEDIAN: four select passes, sums, metrics = 6).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

PASSES = {"lstsq": 3, "median": 6}
THRESHOLDS = (1.25, 1.5625, 1.953125)


def inputs(B, hw, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.rand(B, 1, hw, hw, generator=g, device="cuda") * 0.8 + 0.1
    p = (t - 0.2) / 1.7 + 0.02 * torch.randn(B, 1, hw, hw, generator=g, device="cuda")
    m = torch.rand(B, 1, hw, hw, generator=g, device="cuda") < 0.8
    return p.contiguous(), t.contiguous(), m


def both(x, w=None):
    """[B + 1] sums of x [B, N] (times w): every image, then the batch"""
    s = (x if w is None else x * w).sum(1)
    return torch.cat([s, s.sum()[None]])


def benchmark_fields(al, t, m, min_depth):
    """[B + 1, 7] fp64: fields 8-14 with torch ops"""
    B = al.shape[0]
    mf = m.reshape(B, -1).double()
    ae, te = al.reshape(B, -1).double().clamp(min=min_depth), t.reshape(B, -1).double().clamp(min=min_depth)
    n = both(mf)
    d = ae - te
    ratio = torch.maximum(ae / te, te / ae)
    cols = [both(d.abs() / te, mf) / n, both(d * d / te, mf) / n, (both(d * d, mf) / n).sqrt(),
            (both((ae.log() - te.log()) ** 2, mf) / n).sqrt()]
    cols += [both((ratio < th).double(), mf) / n for th in THRESHOLDS]
    return torch.stack(cols, 1)


def reference_fields(al, t, m):
    """[B + 1, 8] fp64: fields 0-7 (paper_code/evaluation_metrics.py:61-79) with torch ops"""
    B = al.shape[0]
    mf = m.reshape(B, -1).double()
    a, g = al.reshape(B, -1).double(), t.reshape(B, -1).double()
    n = both(mf)
    diff = (a - g).abs() * mf
    dlog = (((1 + 64 * a).log() - (1 + 64 * g).log()) * mf).abs()
    cols = [n, both(diff) / n * 100, both(diff * diff) / n * 100, both((1 + 64 * diff).log(), mf) / n, both(dlog) / n,
            both(dlog * dlog) / n - both(dlog) ** 2 / n ** 2, both(diff / g, mf) / n, both((1 / (1 + 64 * a) - 1 / (1 + 64 * g)) ** 2, mf) / n]
    return torch.stack(cols, 1)


def torch_fit(p, t, m, align):
    """the aligned prediction [B,1,H,W] fp32, clamped, with torch ops (fp64 sums)"""
    B = p.shape[0]
    mf = m.reshape(B, -1).double()
    x, y = p.reshape(B, -1).double(), t.reshape(B, -1).double()
    v = lambda c: c.float().view(B, 1, 1, 1)
    if align == "lstsq":
        n, a00, a01, b0, b1 = mf.sum(1), (mf * x * x).sum(1), (mf * x).sum(1), (mf * x * y).sum(1), (mf * y).sum(1)
        det = a00 * n - a01 * a01
        ok = det != 0
        sc = torch.where(ok, (n * b0 - a01 * b1) / (det + 1e-6), torch.zeros_like(det))
        sh = torch.where(ok, (-a01 * b0 + a00 * b1) / (det + 1e-6), torch.zeros_like(det))
        return (v(sc) * p + v(sh)).clamp(0, 1)
    nan = torch.full_like(x, float("nan"))
    st = []
    for z in (x, y):
        med = torch.where(m.reshape(B, -1), z, nan).nanmedian(1).values.nan_to_num(nan=0.0)
        st += [med, ((z - med[:, None]).abs() * mf).sum(1) / (mf.sum(1) + 1)]
    return ((p - v(st[0])) / (v(st[1]) + 1e-6) * (v(st[3]) + 1e-6) + v(st[2])).clamp(0, 1)


def median_stats(p, t, m):
    """dptx_midas_stats with DPTX_MIDAS_SSI and pred_aligned only (midas_loss._stats would also write target_aligned, which
    the composition does not need) -> stats [B, 8], pred_aligned [B,1,H,W]"""
    from omnidata_amd import midas_loss as ml
    from omnidata_amd._native import call
    from omnidata_amd.engine import _stream
    B, _, H, W = p.shape
    ws = ml._workspace(B, H, W, 1, p.device)
    st = torch.empty(B, ml.STATS, dtype=torch.float32, device=p.device)
    pa = torch.empty_like(p)
    call("dptx_midas_stats", p.data_ptr(), t.data_ptr(), m.view(torch.uint8).data_ptr(), B, H, W, ml.SSI, st.data_ptr(), pa.data_ptr(),
         None, ws.data_ptr(), ws.numel(), _stream(p.device))
    return st, pa


def main():
    from metrics_bench import measure
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,32")
    ap.add_argument("--hw", type=int, default=384)
    ap.add_argument("--align", default="lstsq", choices=sorted(PASSES))
    ap.add_argument("--iters", type=int, default=20, help="calls per window, at least")
    ap.add_argument("--repeats", type=int, default=7, help="windows per measurement")
    ap.add_argument("--min-window-ms", type=float, default=50.0)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("eval_aligned_bench needs an AMD GPU: a timing taken anywhere else says nothing")
    from omnidata_amd import gpu_metrics as gm
    from omnidata_amd import midas_loss as ml
    md = 1e-3
    rows = []
    for B in [int(s) for s in args.sizes.split(",")]:
        p, t, m = inputs(B, args.hw, seed=B)

        def one_call():
            return gm._aligned_rows(p, t, m, args.align, True, md)[0]

        def composition():
            v = lambda c: c.view(B, 1, 1, 1)
            if args.align == "lstsq":
                st = ml._stats(p, t, m, 4, ml.ALIGN)[0]
                al = (v(st[:, 5]) * p + v(st[:, 6])).clamp(0, 1)
            else:
                st, pa = median_stats(p, t, m)
                al = (pa * (v(st[:, 3]) + 1e-6) + v(st[:, 1])).clamp(0, 1)
            first = torch.cat([gm._rows("depth_zbuffer", al, t, m, True), gm._rows("depth_zbuffer", al, t, m, False)])
            return torch.cat([first, benchmark_fields(al, t, m, md)], 1)

        def torch_only():
            al = torch_fit(p, t, m, args.align)
            return torch.cat([reference_fields(al, t, m), benchmark_fields(al, t, m, md)], 1)

        t_ms = measure(dict(one_call=one_call, composition=composition, torch_only=torch_only), args.iters, args.repeats,
                       args.min_window_ms)
        r = dict(align=args.align, B=B, hw=args.hw, valid=int(m.sum()), repeats=args.repeats)
        for name, v in t_ms.items():   # the median of the windows is the figure, min and max its spread
            r[name + "_ms"], r[name + "_ms_min"], r[name + "_ms_max"], r[name + "_calls"] = v["median"], v["min"], v["max"], v["calls"]
        r["one_call_TBps"] = 9 * PASSES[args.align] * B * args.hw * args.hw / (r["one_call_ms"] * 1e-3) / 1e12
        r["speedup_vs_composition"] = r["composition_ms"] / r["one_call_ms"]
        r["speedup_vs_torch_only"] = r["torch_only_ms"] / r["one_call_ms"]
        want = one_call()
        for name, fn in (("composition", composition), ("torch_only", torch_only)):
            r[name + "_worst_diff"] = float(((fn() - want).abs() / want.abs().clamp(min=1.0)).max())
        rows.append(r)
        print(json.dumps(r))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
