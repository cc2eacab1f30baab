"""Times the 3D refocus augmentation: the HIP path (omnidata_amd.refocus.RefocusImageAugmentation) against the same
algorithm written with torch fp32 ops on the same GPU (the reference's method: one replicate-padded depthwise conv pair
per level, the [B, n+1, C, H, W] blur stack, the weighted sum; without its per-image Python threads).

    python tools/refocus_bench.py [--sizes 1,32] [--hw 512] [--n 10] [--iters 10] [--json out.json]

Both paths use the default aperture draw (0.001 .. 6) from the same seed, so they blur the same radii.  HIP events around
`iters` calls after a warm-up; ms per batch and images/s.  Also prints max |HIP - torch fp32| of the timed inputs.
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

from omnidata_amd import refocus as rf  # noqa: E402


def torch_refocus(rgb, depth, n, amin, amax):
    """The reference's computation in torch fp32 on the device (quantiles, draws, blur stack, composite)."""
    B, C, H, W = rgb.shape
    q = torch.quantile(depth.reshape(B, -1), torch.arange(0, n + 1, device=depth.device) / n, dim=1)
    q[0] -= 1e-4
    q[-1] += 1e-4
    q = q.permute(1, 0)
    idx, ap = rf.draw(B, n, amin, amax, depth.device)
    focus = torch.gather(q, 1, idx.unsqueeze(1))
    r = ap * torch.abs(q - focus) / q
    rl = r.tolist()  # the reference reads every radius on the host (int(r * 3))
    stack = []
    for b in range(B):
        levels = []
        img = rgb[b:b + 1]
        for lv in range(n + 1):
            rr = torch.tensor(rl[b][lv], dtype=torch.float32)
            if rr < 0.1:
                levels.append(img)
                continue
            M = int(rr * 3)
            M += 1 - M % 2
            if M == 1:
                levels.append(img)
                continue
            k = torch.arange(0, M, device=rgb.device) - (M - 1.0) / 2.0
            fil = torch.exp(-k ** 2 / (2 * rr.item() * rr.item()))
            s = fil.sum()
            fil = torch.stack([fil] * C)
            p = M // 2
            x = F.pad(img, (p, p, p, p), "replicate")
            x = F.conv2d(x, fil[:, None, None, :], groups=C) / s
            x = F.conv2d(x, fil[:, None, :, None], groups=C) / s
            levels.append(x)
        stack.append(torch.stack(levels, 1))
    stack = torch.cat(stack)
    d = depth.reshape(B, -1)
    right = torch.searchsorted(q, d)
    left = right - 1
    ql, qr = torch.gather(q, 1, left), torch.gather(q, 1, right)
    dl, dr = (d - ql) / (qr - ql), (qr - d) / (qr - ql)
    w = torch.zeros(B, n + 1, H * W, device=rgb.device)
    w.scatter_(1, left.unsqueeze(1), (1 - dl ** 2).unsqueeze(1))
    w.scatter_(1, right.unsqueeze(1), (1 - dr ** 2).unsqueeze(1))
    w /= w.sum(1, keepdim=True)
    return (w.reshape(B, n + 1, 1, H, W) * stack).sum(1)


def time_it(fn, iters):
    fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,32")
    ap.add_argument("--hw", type=int, default=512)
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    results = []
    for B in [int(s) for s in args.sizes.split(",")]:
        g = torch.Generator().manual_seed(B)
        rgb = torch.rand(B, 3, args.hw, args.hw, generator=g).to(dev)
        coarse = torch.rand(B, 1, 8, 8, generator=g) * 4 + 0.2
        depth = F.interpolate(coarse, size=(args.hw, args.hw), mode="bilinear", align_corners=True).contiguous().to(dev)
        aug = rf.RefocusImageAugmentation(args.n, 0.001, 6)

        def hip():
            torch.manual_seed(0)
            return aug(rgb, depth)

        def ref():
            torch.manual_seed(0)
            return torch_refocus(rgb, depth, args.n, 0.001, 6)

        diff = (hip() - ref()).abs().max().item()
        ms_hip = time_it(hip, args.iters)
        ms_ref = time_it(ref, max(1, args.iters // 2))
        row = dict(B=B, H=args.hw, W=args.hw, n=args.n, hip_ms=round(ms_hip, 3), hip_img_s=round(B * 1e3 / ms_hip, 1),
                   torch_fp32_ms=round(ms_ref, 3), torch_fp32_img_s=round(B * 1e3 / ms_ref, 1), max_abs_diff=diff,
                   device=torch.cuda.get_device_name(0))
        print(json.dumps(row), flush=True)
        results.append(row)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
