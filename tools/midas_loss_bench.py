"""Times the MiDaS loss: the HIP path (omnidata_amd.midas_loss.MidasLoss) against the same algorithm written with torch fp32
ops and autograd on the same GPU.

    python tools/midas_loss_bench.py [--sizes 8,32] [--hw 384] [--iters 20] [--json out.json]

Inputs are generated on the device from a seed: a smooth target depth, a prediction that is an affine map of it plus a
smooth field and noise, an 80 % random mask.  HIP events around `iters` calls after two warm-up calls, for the forward
alone and for forward + backward.  Also prints max |HIP - torch fp32| of the losses and of the gradient.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from omnidata_amd import midas_loss as ml  # noqa: E402


def torch_midas(pred, target, mask, alpha=0.1, scales=4):
    """MidasLoss (image-based) in torch fp32 ops: nanmedian alignment + masked L1, inverse depth, least-squares scale and
    shift, four gradient-matching levels."""
    B = pred.shape[0]
    m = mask[:, 0]
    mt = m.float()
    n = m.sum((1, 2))

    def aligned(x):
        t = x[:, 0].masked_fill(~m, float("nan")).reshape(B, -1).nanmedian(-1).values
        t = torch.where(torch.isnan(t), torch.zeros_like(t), t)[:, None, None]
        s = torch.where(m, (x[:, 0] - t).abs(), torch.zeros_like(t)).sum((1, 2)) / (n + 1)
        return (x[:, 0] - t) / (s[:, None, None] + 1e-6)

    ssi = torch.where(m, (aligned(pred) - aligned(target)).abs(), torch.zeros_like(mt)).sum() / m.sum()
    x, y = 1 / (pred[:, 0] + 1e-6), 1 / (target[:, 0] + 1e-6)
    a00, a01, a11 = (mt * x * x).sum((1, 2)), (mt * x).sum((1, 2)), mt.sum((1, 2))
    b0, b1 = (mt * x * y).sum((1, 2)), (mt * y).sum((1, 2))
    det = a00 * a11 - a01 * a01
    ok = det != 0
    scale = torch.where(ok, (a11 * b0 - a01 * b1) / (det + 1e-6), torch.zeros_like(det))
    shift = torch.where(ok, (-a01 * b0 + a00 * b1) / (det + 1e-6), torch.zeros_like(det))
    d = mt * (scale[:, None, None] * x + shift[:, None, None] - y)
    reg = 0
    for k in range(scales):
        s = 2 ** k
        ds, ms = d[:, ::s, ::s], mt[:, ::s, ::s]
        img = ((ms[:, :, 1:] * ms[:, :, :-1]) * (ds[:, :, 1:] - ds[:, :, :-1]).abs()).sum((1, 2)) + \
              ((ms[:, 1:, :] * ms[:, :-1, :]) * (ds[:, 1:, :] - ds[:, :-1, :]).abs()).sum((1, 2))
        M = ms.sum((1, 2))
        reg = reg + torch.where(M != 0, img / M.clamp_min(1), img).mean()
    return ssi + alpha * reg, ssi, reg


def inputs(B, hw, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    def sm(lo, hi):
        f = F.interpolate(torch.rand(B, 1, 6, 6, generator=g, device="cuda"), size=(hw, hw), mode="bilinear", align_corners=True)
        return lo + (hi - lo) * f
    t = sm(0.5, 6.0)
    p = 0.7 * t + 0.3 + 0.5 * sm(0.0, 1.0) + 0.02 * torch.randn(B, 1, hw, hw, generator=g, device="cuda")
    m = torch.rand(B, 1, hw, hw, generator=g, device="cuda") < 0.8
    return p.contiguous(), t.contiguous(), m


def timed(fn, iters):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="8,32")
    ap.add_argument("--hw", type=int, default=384)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    loss = ml.MidasLoss()
    rows = []
    for B in [int(s) for s in args.sizes.split(",")]:
        p, t, m = inputs(B, args.hw, seed=B)
        pg = p.clone().requires_grad_(True)

        def hip_fwd():
            with torch.no_grad():
                return loss(p, t, m)

        def hip_fb():
            pg.grad = None
            loss(pg, t, m)[0].backward()

        def torch_fwd():
            with torch.no_grad():
                return torch_midas(p, t, m)

        def torch_fb():
            pg.grad = None
            torch_midas(pg, t, m)[0].backward()

        r = dict(B=B, hw=args.hw, hip_fwd_ms=timed(hip_fwd, args.iters), hip_fwd_bwd_ms=timed(hip_fb, args.iters),
                 torch_fwd_ms=timed(torch_fwd, args.iters), torch_fwd_bwd_ms=timed(torch_fb, args.iters))
        a, b = torch.stack(hip_fwd()), torch.stack(torch_fwd())
        hip_fb()
        gh = pg.grad.clone()
        torch_fb()
        r.update(max_abs_loss_diff=(a - b).abs().max().item(), max_abs_grad_diff=(gh - pg.grad).abs().max().item(),
                 max_abs_grad=pg.grad.abs().max().item())
        rows.append(r)
        print(json.dumps(r))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
