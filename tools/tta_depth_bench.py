"""Times the alignment and merge of test-time augmentation for depth (dptx_tta_align_depth + dptx_tta_merge_depth) against the same
pipeline composed from torch fp32 ops on the same GPU, and DepthTTA end to end against the plain forwards of the same views.

    python tools/tta_depth_bench.py [--legs a,b] [--repeats 5] [--out profiles/tta_depth_bench.md]

(a) align + merge alone: a 512x683 output, the 40 views of preset "oasis" (maps of 256x352 .. 512x672: a smooth field seen through
    a random scale and shift per view, plus noise), the anchor = the first unflipped whole-image view; B = 1 and 8 images per call.
    `one call` = dptx_tta_align_depth then dptx_tta_merge_depth into preallocated coefficients, workspace and fp32 output;
    `torch` = per image, per view clamp + F.interpolate (+ flip) into a NaN-padded [40,H,W] stack, per view the four sums over its
    window against the anchor's slice and the 2 x 2 solve (on the device, nothing read back), scale * stack + shift, np.median's
    semantics on the device (sort along the views, the mean of the two middle elements by the per-pixel count), clamp, 1 - x.
    Windows between HIP events, at least 50 ms each, the two paths alternating; median (min .. max).
(b) end to end: DepthTTA(model, "oasis", batch_size 32) on B = 1 and 8 images of 512x683 (bf16 DPT-Hybrid, random weights) against
    `forwards`: model(x) on preallocated inputs of the same 40 * B views in the same buckets and batches -- what the network alone
    costs.  Their difference is what upload, view pre-processing, alignment, merge and colouring add.  Host clock around runs
    that end in a device synchronise; runs alternate.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from batch_infer_bench import alternate, clock_note  # noqa: E402

SIZE = (512, 683)   # (H, W)


def _case(B, dev):
    from omnidata_amd import preprocess as pp
    from omnidata_amd.tta import plan_depth_views
    plan, anchor = plan_depth_views(SIZE[1], SIZE[0], "oasis")
    g = torch.Generator(device="cuda").manual_seed(B)
    views, maps, anchors, off = [], [], [], 0
    for i in range(B):
        anchors.append(len(views) + anchor)
        for box, flip, _, (h, w) in plan:
            views.append(pp.TtaView(4 * off, h, w, i, box[1], box[0], box[3] - box[1], box[2] - box[0], int(flip)))
            off += h * w
    flat = torch.empty(off, device=dev)
    for k, v in enumerate(views):
        ys = (v.y0 + (torch.arange(v.h, device=dev) + 0.5) * v.ch / v.h) / SIZE[0]
        xs = (v.x0 + (torch.arange(v.w, device=dev) + 0.5) * v.cw / v.w) / SIZE[1]
        if v.flip:
            xs = xs.flip(0)
        truth = 0.5 + 0.2 * torch.sin(4 * xs[None, :] + ys[:, None]) * torch.cos(3 * ys[:, None] - 2 * xs[None, :])
        a, b = (1.0, 0.0) if k in anchors else (0.8 + 0.45 * float(torch.rand(1, device=dev, generator=g)),
                                                -0.05 + 0.1 * float(torch.rand(1, device=dev, generator=g)))
        m = (truth - b) / a + 0.01 * torch.randn(v.h, v.w, device=dev, generator=g)
        flat[v.offset // 4:v.offset // 4 + v.h * v.w] = m.reshape(-1)
        maps.append(flat[v.offset // 4:v.offset // 4 + v.h * v.w].view(v.h, v.w))
    return views, anchors, flat, maps


def torch_align_merge(maps, views, anchors, B, out):
    """Alignment and merge from torch ops: what a user would write around F.interpolate."""
    H, W = SIZE
    per = len(views) // B
    for i in range(B):
        stack = torch.full((per, H, W), float("nan"), device=out.device)
        for k in range(per):
            v, m = views[i * per + k], maps[i * per + k]
            r = F.interpolate(m.clamp(0, 1)[None, None], (v.ch, v.cw), mode="bilinear", align_corners=False)[0, 0]
            stack[k, v.y0:v.y0 + v.ch, v.x0:v.x0 + v.cw] = r.flip(-1) if v.flip else r
        anchor = anchors[i] - i * per
        scale, shift = [], []
        for k in range(per):
            v = views[i * per + k]
            r = stack[k, v.y0:v.y0 + v.ch, v.x0:v.x0 + v.cw]
            a = stack[anchor, v.y0:v.y0 + v.ch, v.x0:v.x0 + v.cw]
            n = float(v.ch * v.cw)
            sr, srr, sa, sra = r.sum(), (r * r).sum(), a.sum(), (r * a).sum()
            det = n * srr - sr * sr
            ok = det > 1e-10 * n * srr
            one, zero = torch.ones_like(det), torch.zeros_like(det)
            safe = torch.where(ok, det, one)
            s = torch.where(ok, (n * sra - sr * sa) / safe, one)
            t = torch.where(ok, (srr * sa - sr * sra) / safe, (sa - sr) / n)
            scale.append(one if k == anchor else s)
            shift.append(zero if k == anchor else t)
        stack = torch.stack(scale)[:, None, None] * stack + torch.stack(shift)[:, None, None]
        n = (~torch.isnan(stack)).sum(0, keepdim=True)                                # views per pixel
        s = torch.sort(stack, dim=0).values                                          # NaN sorts last
        lo = torch.gather(s, 0, (n - 1).clamp(min=0) // 2)
        hi = torch.gather(s, 0, (n // 2).clamp(max=per - 1))
        out[i].copy_(1 - torch.nan_to_num((lo + hi) * 0.5, nan=0.0)[0].clamp(0, 1))


def leg_a(repeats):
    import ctypes as C
    from omnidata_amd import preprocess as pp
    from omnidata_amd.engine import load_library
    lib = load_library()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    rows = []
    for B in (1, 8):
        views, anchors, flat, maps = _case(B, dev)
        arr = (pp.TtaView * len(views))(*views)
        anc = (C.c_int32 * B)(*anchors)
        descs, total = pp.output_layout([SIZE] * B, "depth_f32")
        nbytes = C.c_int64()
        assert lib.dptx_tta_depth_workspace_bytes(C.addressof(arr), len(views), C.addressof(descs), B, C.byref(nbytes)) == 0
        ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
        coeffs = torch.empty(len(views), 2, device=dev)
        out = torch.empty(total, dtype=torch.uint8, device=dev)
        ref = torch.empty(B, *SIZE, device=dev)

        def kernel():
            assert lib.dptx_tta_align_depth(flat.data_ptr(), C.addressof(arr), len(views), C.addressof(anc), C.addressof(descs), B,
                                            coeffs.data_ptr(), ws.data_ptr(), ws.numel(), stream) == 0
            assert lib.dptx_tta_merge_depth(flat.data_ptr(), C.addressof(arr), len(views), coeffs.data_ptr(), C.addressof(descs), B, 3,
                                            out.data_ptr(), ws.data_ptr(), stream) == 0

        def loop():
            torch_align_merge(maps, views, anchors, B, ref)

        kernel()
        loop()
        torch.cuda.synchronize()
        got = torch.stack([out[d.offset:d.offset + 4 * SIZE[0] * SIZE[1]].view(torch.float32).view(*SIZE) for d in descs[:B]])
        t = alternate(dict(kernel=kernel, loop=loop), repeats)
        rows.append(dict(B=B, views=len(views), map_bytes=flat.numel() * 4, ws_bytes=nbytes.value, kernel=t["kernel"], loop=t["loop"],
                         max_diff=float((got - ref).abs().max())))
        del out, ref, flat, maps, ws
        torch.cuda.empty_cache()
    return rows


def leg_b(repeats):
    from omnidata_amd.model import build_model
    from omnidata_amd.tta import DepthTTA, plan_depth_views
    dev = torch.device("cuda:0")
    model = build_model("depth", random_weights=0, dtype="bf16", max_batch=32).to(dev)
    tta = DepthTTA(model, "oasis", batch_size=32)
    rng = np.random.default_rng(0)
    rows = []
    for B in (1, 8):
        images = [Image.fromarray(rng.integers(0, 256, (*SIZE, 3), dtype=np.uint8)) for _ in range(B)]
        buckets = {}
        for _ in range(B):
            for _, _, _, net in plan_depth_views(SIZE[1], SIZE[0], "oasis")[0]:
                buckets[net] = buckets.get(net, 0) + 1
        order = sorted(buckets, key=lambda net: -net[0] * net[1])
        xs = [torch.rand(min(32, buckets[net] - b0), 3, *net, device=dev) for net in order for b0 in range(0, buckets[net], 32)]

        def end_to_end():
            tta(images)

        def forwards():
            with torch.no_grad():
                for x in xs:
                    model(x)

        got = {"end_to_end": [], "forwards": []}
        for name, fn in (("end_to_end", end_to_end), ("forwards", forwards)):   # the largest shape first: the arena is planned
            fn()
        torch.cuda.synchronize()
        for _ in range(repeats):
            for name, fn in (("end_to_end", end_to_end), ("forwards", forwards)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                got[name].append((time.perf_counter() - t0) * 1e3)
        rows.append(dict(B=B, forwards_n=len(xs), **{k: (statistics.median(v), min(v), max(v)) for k, v in got.items()}))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="a,b")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("tta_depth_bench needs an AMD GPU: a timing taken anywhere else says nothing")
    legs = args.legs.split(",")
    lines = ["# Test-time augmentation for depth: measured", "",
             f"`python tools/tta_depth_bench.py` on {torch.cuda.get_device_name(0)}, 16 host CPUs; clocks after the run: {{clock}}.", ""]

    def fmt(t):
        return f"{t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f})"

    if "a" in legs:
        lines += [f"## (a) Align + merge alone: 40 views per image (preset `oasis`) -> {SIZE[0]}x{SIZE[1]} fp32 depth, median", "",
                  f"Median of {args.repeats} alternating windows between HIP events (min .. max), ms per call.  `one call` = "
                  "`dptx_tta_align_depth` + `dptx_tta_merge_depth`; `torch` = per view clamp + F.interpolate into a NaN-padded "
                  "[40,H,W] stack, 39 sets of four fp32 sums and solves on the device, sort along the views, the two middle "
                  "elements by the per-pixel count, clamp, 1 - x.  `max diff` = the largest difference between the two fp32 results "
                  "(the torch path sums in fp32; tests/test_gpu_tta_depth.py holds the parity check).", "",
                  "| images | views | view maps MB | workspace MB | one call | torch | torch / call | max diff | call faster |",
                  "|---|---|---|---|---|---|---|---|---|"]
        for r in leg_a(args.repeats):
            k, l = r["kernel"], r["loop"]
            lines.append(f"| {r['B']} | {r['views']} | {r['map_bytes'] / 1e6:.0f} | {r['ws_bytes'] / 1e6:.1f} | {fmt(k)} | {fmt(l)} | "
                         f"{l[0] / k[0]:.1f}x | {r['max_diff']:.1e} | {'yes' if k[0] < l[0] else 'NO'} |")
            print(lines[-1], flush=True)
        lines.append("")
    if "b" in legs:
        lines += [f"## (b) End to end: DepthTTA(`oasis`, batch_size 32) on {SIZE[0]}x{SIZE[1]} RGB images, bf16 DPT-Hybrid", "",
                  f"Median of {args.repeats} alternating runs (min .. max), ms per call; host clock around runs that end in a device "
                  "synchronise.  `forwards` = model(x) alone on preallocated inputs of the same views in the same batches; "
                  "`pre + align + merge share` = (end to end - forwards) / end to end: upload, view inputs, the copies of the maps, "
                  "alignment, merge, colouring.", "",
                  "| images | forwards per call | end to end | forwards | pre + align + merge share |", "|---|---|---|---|---|"]
        for r in leg_b(args.repeats):
            e, f = r["end_to_end"], r["forwards"]
            lines.append(f"| {r['B']} | {r['forwards_n']} | {fmt(e)} | {fmt(f)} | {100 * (e[0] - f[0]) / e[0]:.1f} % |")
            print(lines[-1], flush=True)
        lines.append("")
    text = "\n".join(lines).replace("{clock}", clock_note())
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
