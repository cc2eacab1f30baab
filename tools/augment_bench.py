"""Times the training augmentations (omnidata_amd/augmentation.py over csrc/augment.hip) against the same operations composed from
torch ops on the same GPU (the code of tests/augment_restatement.py on device tensors), and the blur chain against a plain device
copy of the same bytes.

    python tools/augment_bench.py [--repeats 5] [--out profiles/augment_bench.md]

3 x 384 x 384 and 3 x 512 x 512 images, B = 1 and 32.  The chain with all three stages at their largest sizes (motion 7 x 7,
Gaussian 7 x 7), each stage alone, and resize_tasks (rgb bilinear, a depth map and a bool mask nearest: 512 x 512 -> 384 x 384, and
the 384 x 384 crop).  The kernel rows time the launch alone (tables uploaded before); `call` adds the host plan and the upload.
Windows between HIP events, at least 50 ms each, the paths alternating; the figure is the median, min..max its spread.  Behind
the table, what bounds the chain: the time its FMAs, its LDS reads and its memory traffic would each take alone at peak rate."""
from __future__ import annotations

import argparse
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from batch_infer_bench import alternate, clock_note  # noqa: E402

SIZES = [(384, 384), (512, 512)]
BATCHES = [1, 32]
# MI355X: 256 CUs of 4 SIMDs at 2.4 GHz, a wave64 VALU instruction over 2 cycles; 128 bytes of LDS per CU and clock; 8 TB/s of HBM
CUS, CLOCK_HZ, LDS_BYTES_PER_CLK, HBM_BYTES_PER_S, VALU_CYCLES = 256, 2.4e9, 128, 8.0e12, 2
TW, TH, V = 64, 32, 4      # csrc/augment.hip


def stage_work(stages):
    """(fma, LDS reads) per OUTPUT pixel of the chain with the given stages (k per stage, None = off), the halo regions of the
    earlier stages included: a stage computes (TH + 2 h)(TW + 2 h) pixels of a tile, h the halo the stages behind it need."""
    ks = [k for k in stages if k]
    fma = reads = 0.0
    for i, k in enumerate(ks):
        h = sum(x // 2 for x in ks[i + 1:])
        area = (TH + 2 * h) * (TW + 2 * h) / (TH * TW)
        fma += area * k * k
        reads += area * (V + k - 1) * k / V
    return fma, reads


def bounds_ms(n, stages):
    fma, reads = stage_work(stages)
    valu = n * fma * VALU_CYCLES / 64 / (CUS * 4 * CLOCK_HZ) * 1e3
    lds = n * reads * 4 / (CUS * LDS_BYTES_PER_CLK * CLOCK_HZ) * 1e3
    mem = n * 8 / HBM_BYTES_PER_S * 1e3
    return valu, lds, mem


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("augment_bench needs an AMD GPU: a timing taken anywhere else says nothing")
    import augment_restatement as R
    from omnidata_amd import augmentation as A
    dev = torch.device("cuda:0")
    fmt = lambda t: f"{t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f})"
    lines = ["# Training augmentations: measured", "",
             f"`python tools/augment_bench.py` on {torch.cuda.get_device_name(0)}, 16 host CPUs; clocks after the run: {{clock}}.", "",
             f"Median of {args.repeats} alternating windows between HIP events (min .. max), ms per batch.  `kernel` = the one launch with "
             "the tables already on the device; `call` = `filter_chain` with Python parameters (host tables, one pinned upload, the "
             "launch); `torch ops` = the same definition composed from torch fp32 ops on the same GPU; `copy` = `out.copy_(x)`.", "",
             "## The blur chain (sharpness, motion 7 x 7, Gaussian 7 x 7) and its stages alone", "",
             "| stages | batch | kernel | call | torch ops | torch / kernel | copy | kernel / copy |", "|---|---|---|---|---|---|---|---|"]
    bound_rows = []
    for (H, W), B in [(s, b) for s in SIZES for b in BATCHES]:
        g = torch.Generator(device="cuda").manual_seed(H + B)
        x = torch.rand(B, 3, H, W, device=dev, generator=g)
        out = torch.empty_like(x)
        cpu = torch.Generator().manual_seed(B)
        u = lambda: torch.rand(B, generator=cpu).double()
        full = dict(sharpness=(u() * 0.3).tolist(), motion=(7, ((2 * u() - 1) * 50).tolist(), ((2 * u() - 1) * 0.5).tolist()),
                    gaussian=(7, (0.1 + 1.9 * u()).tolist()))
        for name, keys, ks in (("all three", ("sharpness", "motion", "gaussian"), (3, 7, 7)), ("sharpness", ("sharpness",), (3, 0, 0)),
                               ("motion 7 x 7", ("motion",), (0, 7, 0)), ("Gaussian 7 x 7", ("gaussian",), (0, 0, 7))):
            p = {k: full[k] for k in keys}
            plan = A.plan_filter_chain(B, **p)
            tables = A.upload(plan, dev)
            rs = None if tables.sharp is None else tables.sharp
            rg = None if tables.gy is None else (tables.gy, tables.gx)
            t = alternate(dict(kernel=lambda: A.filter_chain(x, tables=tables, out=out), call=lambda: A.filter_chain(x, out=out, **p),
                               torch=lambda: R.chain(x, rs, tables.motion, rg), copy=lambda: out.copy_(x)), args.repeats)
            lines.append(f"| {name} | {B} x 3 x {H} x {W} | {fmt(t['kernel'])} | {fmt(t['call'])} | {fmt(t['torch'])} | "
                         f"{t['torch'][0] / t['kernel'][0]:.1f}x | {fmt(t['copy'])} | {t['kernel'][0] / t['copy'][0]:.1f}x |")
            print(lines[-1], flush=True)
            if B == 32:
                bound_rows.append((name, H, W, t["kernel"][0], bounds_ms(x.numel(), ks)))
        del x, out
        torch.cuda.empty_cache()
    lines += ["", "What bounds the chain kernel at B = 32: the time each resource would take alone at its peak rate (256 CUs of 4 SIMDs at "
              "2.4 GHz, 2 cycles per wave64 FMA, the halo regions of the earlier stages included; 128 B of LDS per CU and clock, "
              f"(V + k - 1) k / V reads per output with V = {V}; 8 TB/s of HBM for one read and one write), next to the measured time.", "",
              "| stages | image | measured | FMAs alone | LDS reads alone | memory alone |", "|---|---|---|---|---|---|"]
    for name, H, W, ms, (v, l, m) in bound_rows:
        lines.append(f"| {name} | {H} x {W} | {ms:.3f} | {v:.3f} | {l:.3f} | {m:.3f} |")
        print(lines[-1], flush=True)

    lines += ["", "## resize_tasks: rgb [B,3,512,512] fp32 (bilinear), depth [B,1,512,512] fp32 and a bool mask [B,1,512,512] (nearest)", "",
              "`torch ops` = `F.interpolate` per task (the mask through uint8) / a slice made contiguous per task.", "",
              "| operation | batch | one launch | torch ops | torch / launch | GB/s moved (launch) |", "|---|---|---|---|---|---|"]
    for B in BATCHES:
        g = torch.Generator(device="cuda").manual_seed(B)
        batch = {"rgb": torch.rand(B, 3, 512, 512, device=dev, generator=g), "depth_zbuffer": torch.rand(B, 1, 512, 512, device=dev, generator=g),
                 "mask_valid": torch.rand(B, 1, 512, 512, device=dev, generator=g) < 0.5}
        names = list(batch)

        def torch_resize():
            return [F.interpolate(batch["rgb"], (384, 384), mode="bilinear"), F.interpolate(batch["depth_zbuffer"], (384, 384), mode="nearest"),
                    F.interpolate(batch["mask_valid"].view(torch.uint8), (384, 384), mode="nearest").view(torch.bool)]

        def torch_crop():
            return [batch[k][:, :, 64:448, 64:448].contiguous() for k in names]

        for op, ours, theirs in (("resize -> 384 x 384", lambda: A.resize_tasks(batch, names, "resize", (384, 384)), torch_resize),
                                 ("crop 384 x 384", lambda: A.resize_tasks(batch, names, "crop", (384, 384), (64, 64)), torch_crop)):
            t = alternate(dict(ours=ours, theirs=theirs), args.repeats)
            moved = 2 * B * 384 * 384 * (3 * 4 + 4 + 1)
            lines.append(f"| {op} | {B} | {fmt(t['ours'])} | {fmt(t['theirs'])} | {t['theirs'][0] / t['ours'][0]:.1f}x | "
                         f"{moved / (t['ours'][0] * 1e-3) / 1e9:.0f} |")
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
