"""Times the surface-normal loss: the HIP path (omnidata_amd.normal_loss.NormalLoss) against the same objective written with
torch fp32 ops and autograd on the same GPU, the way the reference writes it.

    python tools/normal_loss_bench.py [--sizes 1,32] [--hw 384] [--iters 20] [--json out.json]
    python tools/normal_loss_bench.py --check-cpu          # the torch path against tests/golden/normal_*.npz, no GPU

Inputs are generated on the device from a seed: targets 0.5 n + 0.5 for random unit n, the prediction the target plus
noise (some of it outside [0, 1]: the objective clamps), an 80 % mask.  The torch path follows train_normal.py:251-258 and
losses/masked_losses.py step by step: clamp, the mask repeated over the channels, |p - t| zeroed outside the mask in place,
the permute and the boolean compaction of the cosine loss (a device-to-host synchronisation), F.normalize.  HIP events
around `iters` calls after two warm-up calls, forward alone and forward + backward.  Also prints the achieved bytes per
second of the HIP path (25 B per pixel read forward; the backward reads them again and writes 12 B per pixel) and the
differences of the losses and of the gradients.
"""
from __future__ import annotations

import argparse
import glob
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_normal_loss(pred, target, mask, l1_weight=10.0, clamp_pred=True):
    """train_normal.py:251-258 in torch ops; mask [B,1,H,W] bool -> (total, l1, cos)"""
    p = torch.clamp(pred, 0, 1) if clamp_pred else pred
    m3 = mask.repeat_interleave(3, 1)
    e = abs(p - target)
    e[~m3] = 0
    l1 = e.sum() / m3.sum()
    a = (2 * p - 1).clamp(-1, 1)
    b = (2 * target - 1).clamp(-1, 1)
    mv = m3[:, 0, :, :].bool()
    a = a.permute(0, 2, 3, 1)[mv, :]              # boolean compaction: the device-to-host synchronisation of the reference
    b = b.permute(0, 2, 3, 1)[mv, :]
    cos = torch.mean(-torch.sum(F.normalize(a, p=2, dim=1) * F.normalize(b, p=2, dim=1), dim=1))
    return cos + l1_weight * l1, l1, cos


def check_cpu():
    """the torch path against the goldens of the reference, on the CPU: losses to 1e-6, gradients to 1e-5 of their maximum"""
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "normal_*.npz"))):
        z = np.load(path)
        if "losses" not in z.files:
            continue
        pred = torch.from_numpy(z["pred"]).requires_grad_(True)
        out = torch_normal_loss(pred, torch.from_numpy(z["target"]), torch.from_numpy(z["mask"]), float(z["l1_weight"]),
                                bool(int(z["flags"]) & 4))
        got = torch.stack(out).detach().numpy()
        assert np.allclose(got, z["losses"], rtol=1e-6, atol=1e-6, equal_nan=True), (path, got, z["losses"])
        if not np.isnan(got).any():
            out[0].backward()
            gmax = np.abs(z["grad_total"]).max()
            assert np.abs(pred.grad.numpy() - z["grad_total"]).max() <= 1e-5 * gmax, path
        print(f"{os.path.basename(path)}: torch path = reference {got.tolist()}")


def inputs(B, hw, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    n = torch.randn(B, 3, hw, hw, generator=g, device="cuda")
    t = 0.5 * n / n.norm(dim=1, keepdim=True) + 0.5
    p = t + 0.2 * torch.randn(B, 3, hw, hw, generator=g, device="cuda")
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
    ap.add_argument("--sizes", default="1,32")
    ap.add_argument("--hw", type=int, default=384)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default="")
    ap.add_argument("--check-cpu", action="store_true")
    args = ap.parse_args()
    if args.check_cpu:
        check_cpu()
        return
    from omnidata_amd.normal_loss import NormalLoss
    loss = NormalLoss()
    rows = []
    for B in [int(s) for s in args.sizes.split(",")]:
        pred, gt, mask = inputs(B, args.hw, seed=B)
        pg = pred.clone().requires_grad_(True)

        def hip_fwd():
            with torch.no_grad():
                return loss(pred, gt, mask)["normal_loss"]

        def hip_fb():
            pg.grad = None
            loss(pg, gt, mask)["normal_loss"].backward()

        def torch_fwd():
            with torch.no_grad():
                return torch_normal_loss(pred, gt, mask)[0]

        def torch_fb():
            pg.grad = None
            torch_normal_loss(pg, gt, mask)[0].backward()

        px = B * args.hw * args.hw
        r = dict(B=B, hw=args.hw, hip_fwd_ms=timed(hip_fwd, args.iters), hip_fwd_bwd_ms=timed(hip_fb, args.iters),
                 torch_fwd_ms=timed(torch_fwd, args.iters), torch_fwd_bwd_ms=timed(torch_fb, args.iters))
        r["hip_fwd_TBps"] = 25 * px / (r["hip_fwd_ms"] * 1e-3) / 1e12
        r["hip_fwd_bwd_TBps"] = (25 + 25 + 12) * px / (r["hip_fwd_bwd_ms"] * 1e-3) / 1e12
        a, b = hip_fwd(), torch_fwd()
        hip_fb()
        gh = pg.grad.clone()
        torch_fb()
        r.update(valid=int(mask.sum()), hip_loss=a.item(), torch_loss=b.item(), max_abs_grad_diff=(gh - pg.grad).abs().max().item(),
                 max_abs_grad=pg.grad.abs().max().item())
        rows.append(r)
        print(json.dumps(r))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
