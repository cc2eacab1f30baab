"""Times the merge of test-time augmentation (dptx_tta_merge_normals) against the same result composed from torch ops on the same
GPU, and NormalsTTA end to end against the plain forwards of the same views.

    python tools/tta_bench.py [--legs a,b] [--repeats 5] [--out profiles/tta_bench.md]

(a) merge alone: a 512x683 output, the 40 views of preset "oasis" (maps of 256x352 .. 512x672, random values), B = 1 and 8
    images per call.  `one call` = dptx_tta_merge_normals into a preallocated uint8 output; `torch` = per image, per view
    decode + F.normalize + F.interpolate (+ flip and x negation) into a NaN-padded [40,3,H,W] stack, np.median's semantics
    on the device (sort along the views, the mean of the two middle elements by the per-pixel count; torch.nanmedian is the
    lower median), F.normalize, encode, quantise.  Windows between HIP events, at least 50 ms each, the two paths alternating; median (min .. max).
(b) end to end: NormalsTTA(model, "oasis", batch_size 32) on B = 1 and 8 images of 512x683 (bf16 DPT-Hybrid, random weights)
    against `forwards`: model(x) on preallocated inputs of the same 40 * B views in the same buckets and batches -- what the
    network alone costs.  Their difference is what upload, view pre-processing and merge add.  Host clock around runs that end
    in a device synchronise; runs alternate.
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
    from omnidata_amd.tta import plan_views
    plan = plan_views(SIZE[1], SIZE[0], "oasis")
    g = torch.Generator(device="cuda").manual_seed(B)
    views, maps, off = [], [], 0
    for i in range(B):
        for box, flip, _, (h, w) in plan:
            views.append(pp.TtaView(4 * off, h, w, i, box[1], box[0], box[3] - box[1], box[2] - box[0], int(flip)))
            off += 3 * h * w
    flat = torch.rand(off, device=dev, generator=g)
    for v in views:
        maps.append(flat[v.offset // 4:v.offset // 4 + 3 * v.h * v.w].view(3, v.h, v.w))
    return plan, views, flat, maps


def torch_merge(maps, views, B, out):
    """The merge from torch ops: what a user would write around F.interpolate."""
    H, W = SIZE
    per = len(views) // B
    for i in range(B):
        stack = torch.full((per, 3, H, W), float("nan"), device=out.device)
        for k in range(per):
            v, m = views[i * per + k], maps[i * per + k]
            r = F.interpolate(F.normalize(2 * m - 1, dim=0)[None], (v.ch, v.cw), mode="bilinear", align_corners=False)[0]
            if v.flip:
                r = r.flip(-1)
                r[0] = -r[0]
            stack[k, :, v.y0:v.y0 + v.ch, v.x0:v.x0 + v.cw] = r
        n = (~torch.isnan(stack[:, :1])).sum(0, keepdim=True)                       # views per pixel
        s = torch.sort(stack, dim=0).values                                        # NaN sorts last
        lo = torch.gather(s, 0, ((n - 1).clamp(min=0) // 2).expand(1, 3, H, W))
        hi = torch.gather(s, 0, (n // 2).clamp(max=per - 1).expand(1, 3, H, W))
        med = torch.nan_to_num((lo + hi) * 0.5, nan=0.0)[0]
        out[i].copy_(((F.normalize(med, dim=0) + 1) / 2).clamp(0, 1).mul(255).byte().permute(1, 2, 0))


def leg_a(repeats):
    import ctypes as C
    from omnidata_amd import preprocess as pp
    from omnidata_amd.engine import load_library
    lib = load_library()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    rows = []
    for B in (1, 8):
        plan, views, flat, maps = _case(B, dev)
        arr = (pp.TtaView * len(views))(*views)
        descs, total = pp.output_layout([SIZE] * B, "normal_u8")
        out = torch.empty(total, dtype=torch.uint8, device=dev)
        ref = torch.empty(B, *SIZE, 3, dtype=torch.uint8, device=dev)

        def kernel():
            assert lib.dptx_tta_merge_normals(flat.data_ptr(), C.addressof(arr), len(views), C.addressof(descs), B, 1, out.data_ptr(),
                                              stream) == 0

        def loop():
            torch_merge(maps, views, B, ref)

        kernel()
        loop()
        torch.cuda.synchronize()
        got = torch.stack([out[d.offset:d.offset + SIZE[0] * SIZE[1] * 3].view(*SIZE, 3) for d in descs[:B]])
        diff = (got.int() - ref.int()).abs()
        t = alternate(dict(kernel=kernel, loop=loop), repeats)
        rows.append(dict(B=B, views=len(views), map_bytes=flat.numel() * 4, kernel=t["kernel"], loop=t["loop"],
                         max_diff=int(diff.max()), frac_diff=float((diff > 0).float().mean())))
        del out, ref, flat, maps
        torch.cuda.empty_cache()
    return rows


def leg_b(repeats):
    from omnidata_amd.model import build_model
    from omnidata_amd.tta import NormalsTTA, plan_views
    dev = torch.device("cuda:0")
    model = build_model("normal", random_weights=0, dtype="bf16", max_batch=32).to(dev)
    tta = NormalsTTA(model, "oasis", batch_size=32)
    rng = np.random.default_rng(0)
    rows = []
    for B in (1, 8):
        images = [Image.fromarray(rng.integers(0, 256, (*SIZE, 3), dtype=np.uint8)) for _ in range(B)]
        buckets = {}
        for _ in range(B):
            for _, _, _, net in plan_views(SIZE[1], SIZE[0], "oasis"):
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
        raise RuntimeError("tta_bench needs an AMD GPU: a timing taken anywhere else says nothing")
    legs = args.legs.split(",")
    lines = ["# Test-time augmentation for surface normals: measured", "",
             f"`python tools/tta_bench.py` on {torch.cuda.get_device_name(0)}, 16 host CPUs; clocks after the run: {{clock}}.", ""]

    def fmt(t):
        return f"{t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f})"

    if "a" in legs:
        lines += [f"## (a) The merge alone: 40 views per image (preset `oasis`) -> {SIZE[0]}x{SIZE[1]} uint8 normals, median", "",
                  f"Median of {args.repeats} alternating windows between HIP events (min .. max), ms per call.  `torch` = per view normalize + "
                  "F.interpolate into a NaN-padded [40,3,H,W] stack, sort along the views, the two middle elements by the per-pixel "
                  "count, normalize, quantise.  `levels` = the largest difference between the two uint8 results and the share of "
                  "bytes that differ (the two round differently; tests/test_gpu_tta.py holds the parity check).", "",
                  "| images | views | view maps MB | one call | torch | torch / call | levels | call faster |", "|---|---|---|---|---|---|---|---|"]
        for r in leg_a(args.repeats):
            k, l = r["kernel"], r["loop"]
            lines.append(f"| {r['B']} | {r['views']} | {r['map_bytes'] / 1e6:.0f} | {fmt(k)} | {fmt(l)} | {l[0] / k[0]:.1f}x | "
                         f"{r['max_diff']} ({100 * r['frac_diff']:.3f} %) | {'yes' if k[0] < l[0] else 'NO'} |")
            print(lines[-1], flush=True)
        lines.append("")
    if "b" in legs:
        lines += [f"## (b) End to end: NormalsTTA(`oasis`, batch_size 32) on {SIZE[0]}x{SIZE[1]} RGB images, bf16 DPT-Hybrid", "",
                  f"Median of {args.repeats} alternating runs (min .. max), ms per call; host clock around runs that end in a device "
                  "synchronise.  `forwards` = model(x) alone on preallocated inputs of the same views in the same batches; "
                  "`pre + merge share` = (end to end - forwards) / end to end: upload, view inputs, the copies of the maps, the merge.", "",
                  "| images | forwards per call | end to end | forwards | pre + merge share |", "|---|---|---|---|---|"]
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
