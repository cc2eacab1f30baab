"""Times the virtual normal loss: the HIP path (omnidata_amd.virtual_normal_loss.VNL_Loss) against the same algorithm written
with torch fp32 ops and autograd on the same GPU.

    python tools/vnl_loss_bench.py [--sizes 1,32] [--hw 384] [--iters 20] [--json out.json]

Inputs are generated on the device from a seed: a smooth depth in [0.05, 1] and a second one that is it plus a smooth
field and noise; fx = fy = 1 and the call order of train_depth.py (the prediction first, the gradient with respect to it).
One draw of triples (np.random.seed) serves every call of both paths, so the draw itself is not timed.  The torch path
follows the reference's steps: [B, n, 3, 3] groups, the 3x3 bmm, boolean compaction (a device-to-host synchronisation)
and torch.sort.  HIP events around `iters` calls after two warm-up calls, forward alone and forward + backward.  Also
prints the difference of the losses and of the gradients.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from omnidata_amd import virtual_normal_loss as vl  # noqa: E402


def torch_vnl(first, second, p, fx=1.0, fy=1.0, delta_z=1e-4, select=True):
    """VNL_Loss.forward in torch fp32 ops; p: three int64 tensors [n] of linear pixel indices on the device"""
    B, _, H, W = first.shape
    dev = first.device
    u = (torch.arange(W, device=dev, dtype=torch.float32) - W // 2)[None, None, :].expand(1, H, W)
    v = (torch.arange(H, device=dev, dtype=torch.float32) - H // 2)[None, :, None].expand(1, H, W)

    def groups(d):
        pw = torch.stack([u * d[:, 0].abs() / fx, v * d[:, 0].abs() / fy, d[:, 0]], -1).reshape(B, H * W, 3)
        return torch.stack([pw[:, p[0]], pw[:, p[1]], pw[:, p[2]]], 3)   # [B, n, 3 (xyz), 3 (point)]

    g1, g2 = groups(first), groups(second)
    diff = torch.stack([g1[..., 1] - g1[..., 0], g1[..., 2] - g1[..., 0], g1[..., 2] - g1[..., 1]], 3)
    n = diff.shape[1]
    q = diff.reshape(B * n, 3, 3).permute(0, 2, 1)
    k = diff.reshape(B * n, 3, 3)
    qn = q.norm(2, dim=2)
    nm = torch.bmm(qn.view(B * n, 3, 1), qn.view(B * n, 1, 3))
    e = (torch.bmm(q, k) / (nm + 1e-8)).view(B * n, -1)
    mask_cos = (((e > 0.867) + (e < -0.867)).sum(1) > 3).view(B, n)
    mask_pad = (g1[:, :, 2, :] > delta_z).sum(2) == 3
    near = [(diff[:, :, c, :].abs() < 0.005).sum(2) > 0 for c in range(3)]
    mask = mask_pad & ~((near[0] & near[1] & near[2]) | mask_cos)
    g2 = g2.clone()
    g2[g2[:, :, 2, :] == 0] = 0.0001
    a = g1[mask].reshape(1, -1, 3, 3)          # boolean compaction: the device-to-host synchronisation of the reference
    b = g2[mask].reshape(1, -1, 3, 3)

    def unit(x):
        nrm = torch.cross(x[..., 1] - x[..., 0], x[..., 2] - x[..., 0], dim=2)
        s = nrm.norm(2, dim=2, keepdim=True)
        return nrm / (s + (s == 0).float() * 0.01)

    loss = (unit(a) - unit(b)).abs().sum(2).sum(0)
    if select:
        loss, _ = torch.sort(loss, dim=0, descending=False)
        loss = loss[int(loss.size(0) * 0.25):]
    return loss.mean()


def inputs(B, hw, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)

    def sm(lo, hi):
        f = F.interpolate(torch.rand(B, 1, 6, 6, generator=g, device="cuda"), size=(hw, hw), mode="bilinear", align_corners=True)
        return lo + (hi - lo) * f
    t = sm(0.05, 1.0)
    p = (0.8 * t + 0.2 * sm(0.05, 1.0) + 0.01 * torch.randn(B, 1, hw, hw, generator=g, device="cuda")).clamp(0.02, 1.5)
    return p.contiguous(), t.contiguous()


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
    ap.add_argument("--sizes", default="1,32")
    ap.add_argument("--hw", type=int, default=384)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    loss = vl.VNL_Loss(1.0, 1.0, (args.hw, args.hw))
    np.random.seed(0)
    p123 = loss.select_index()
    lin = [torch.from_numpy(p123[f"p{j}_y"].astype(np.int64) * args.hw + p123[f"p{j}_x"].astype(np.int64)).cuda() for j in (1, 2, 3)]
    rows = []
    for B in [int(s) for s in args.sizes.split(",")]:
        pred, gt = inputs(B, args.hw, seed=B)
        pg = pred.clone().requires_grad_(True)

        def hip_fwd():
            with torch.no_grad():
                return loss(pred, gt, p123=p123)

        def hip_fb():
            pg.grad = None
            loss(pg, gt, p123=p123).backward()

        def torch_fwd():
            with torch.no_grad():
                return torch_vnl(pred, gt, lin)

        def torch_fb():
            pg.grad = None
            torch_vnl(pg, gt, lin).backward()

        r = dict(B=B, hw=args.hw, n=int(lin[0].numel()), hip_fwd_ms=timed(hip_fwd, args.iters), hip_fwd_bwd_ms=timed(hip_fb, args.iters),
                 torch_fwd_ms=timed(torch_fwd, args.iters), torch_fwd_bwd_ms=timed(torch_fb, args.iters))
        a, b = hip_fwd(), torch_fwd()
        hip_fb()
        gh = pg.grad.clone()
        torch_fb()
        r.update(K=loss.diagnostics(pred, gt, p123)["K"], hip_loss=a.item(), torch_loss=b.item(),
                 max_abs_grad_diff=(gh - pg.grad).abs().max().item(), max_abs_grad=pg.grad.abs().max().item())
        rows.append(r)
        print(json.dumps(r))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
