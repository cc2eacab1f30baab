"""Times the two full-frame entry points against the same result in torch ops on the same GPU, and a folder of PNGs through
BatchPredictor.predict_to_dir with full_frame "squash" / "aspect" against full_frame=None.

    python tools/fullframe_bench.py [--legs a,b,c] [--repeats 5] [--folder-repeats 3] [--images 256] [--out profiles/fullframe_bench.md]

(a) post: y [32,3,384,512] (normals) and [32,1,384,512] (depth) -> 32 outputs of the originals' size (512x640, 1080x1920,
    3000x4000): one dptx_postprocess_resize_batch call against a per-image loop of F.interpolate + clamp + mul + byte + permute
    (normals) or F.interpolate(bicubic) + clamp + 1-x (depth) into preallocated outputs.  Windows between HIP events, at least
    50 ms each, the two paths alternating; the figure is the median, min..max its spread.
(b) pre: 32 device-resident RGB images of those sizes -> x [32,3,384,512]: one dptx_preprocess_u8_rect_batch call, the same
    way; for reference only, 32 PIL resizes of the same images on the host (host clock, one run).
(c) a folder of PNGs (512x640) written at run time: predict_to_dir with full_frame=None, "squash" and "aspect", batch_size 32,
    bf16.  Host clock around runs that end in a device synchronise; runs alternate.
"""
from __future__ import annotations

import argparse
import ctypes as C
import glob
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch
import torch.nn.functional as F
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from batch_infer_bench import alternate, clock_note, make_folder  # noqa: E402

SHAPES = [(512, 640), (1080, 1920), (3000, 4000)]
NET = (384, 512)
B = 32


def leg_a(repeats):
    from omnidata_amd import preprocess as pp
    from omnidata_amd._native import workspace
    from omnidata_amd.engine import load_library
    lib = load_library()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    lut = torch.from_numpy(pp.viridis_lut()).to(dev)
    rows = []
    for mode, code, Cn in (("normal_u8", 1, 3), ("normal_u8+renorm", 17, 3), ("depth_f32", 3, 1), ("depth_rgba", 4, 1)):
        y = torch.rand(B, Cn, *NET, device=dev) * 1.4 - 0.2
        ws = workspace("dptx_postprocess_resize_workspace_bytes", dev, (B, 4), "unsupported")
        for H, W in SHAPES:
            base = mode.split("+")[0]
            descs, total = pp.output_layout([(H, W)] * B, base)
            out = torch.empty(total, dtype=torch.uint8, device=dev)

            def kernel():
                assert lib.dptx_postprocess_resize_batch(y.data_ptr(), B, Cn, NET[0], NET[1], C.addressof(descs), code, out.data_ptr(),
                                                         lut.data_ptr(), ws.data_ptr(), ws.numel(), stream) == 0

            if base == "normal_u8":
                ref = torch.empty(B, H, W, 3, dtype=torch.uint8, device=dev)

                def loop():
                    for i in range(B):
                        v = F.interpolate(y[i:i + 1], (H, W), mode="bilinear", align_corners=False)
                        if code & 16:
                            v = (F.normalize(2 * v - 1, dim=1) + 1) / 2
                        ref[i].copy_(v.clamp(0, 1).mul(255).byte()[0].permute(1, 2, 0))
            elif base == "depth_f32":
                ref = torch.empty(B, H, W, device=dev)

                def loop():
                    for i in range(B):
                        ref[i].copy_(1 - F.interpolate(y[i:i + 1], (H, W), mode="bicubic", align_corners=False).clamp(0, 1)[0, 0])
            else:
                ref = torch.empty(B, H, W, 4, dtype=torch.uint8, device=dev)
                lut_rows = lut.view(256, 4)

                def loop():
                    for i in range(B):
                        v = 1 - F.interpolate(y[i:i + 1], (H, W), mode="bicubic", align_corners=False).clamp(0, 1)[0, 0]
                        lo, hi = v.min(), v.max()
                        idx = ((v - lo) / (hi - lo) * 256).clamp(0, 255).long()
                        ref[i].copy_(lut_rows[idx])
            t = alternate(dict(kernel=kernel, loop=loop), repeats)
            rows.append(dict(mode=mode, shape=f"{H}x{W}", bytes=total, kernel=t["kernel"], loop=t["loop"]))
            del out, ref
            torch.cuda.empty_cache()
    return rows


def leg_b(repeats):
    from omnidata_amd import preprocess as pp
    from omnidata_amd._native import workspace
    from omnidata_amd.engine import load_library
    lib = load_library()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    ws = workspace("dptx_preprocess_rect_batch_workspace_bytes", dev, (B, *NET), "unsupported")
    x = torch.empty(B, 3, *NET, device=dev)
    rows = []
    for H, W in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(H)
        one = (H * W * 3 + 15) // 16 * 16
        packed = torch.randint(0, 256, (B * one,), dtype=torch.uint8, device=dev, generator=g)
        descs = (pp.ImageDesc * B)(*[pp.ImageDesc(i * one, H, W, 3, W * 3) for i in range(B)])

        def kernel():
            assert lib.dptx_preprocess_u8_rect_batch(packed.data_ptr(), C.addressof(descs), B, NET[0], NET[1], 0, x.data_ptr(),
                                                     ws.data_ptr(), ws.numel(), stream) == 0

        t = alternate(dict(kernel=kernel), repeats)
        imgs = [Image.fromarray(packed[i * one:i * one + H * W * 3].view(H, W, 3).cpu().numpy()) for i in range(4)]
        t0 = time.perf_counter()
        for im in imgs:
            pp.to_tensor(im.resize((NET[1], NET[0]), Image.BILINEAR))
        pil_ms = (time.perf_counter() - t0) * 1e3 * (B / len(imgs))
        rows.append(dict(shape=f"{H}x{W}", bytes=B * H * W * 3, kernel=t["kernel"], pil_ms=pil_ms))
        del packed
        torch.cuda.empty_cache()
    return rows


def leg_c(n_images, repeats, batch=32):
    from omnidata_amd.batch_infer import BatchPredictor
    from omnidata_amd.model import build_model
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "in")
        os.makedirs(src)
        make_folder(src, n_images)
        files = sorted(glob.glob(src + "/*"))
        model = build_model("normal", random_weights=0, dtype="bf16", max_batch=batch).to("cuda:0")
        preds = {str(ff): BatchPredictor(model, "normal", batch_size=batch, full_frame=ff) for ff in ("aspect", "squash", None)}
        outs = {k: os.path.join(tmp, k) for k in preds}
        for k, bp in preds.items():   # the largest network shape first: the arena is planned before the runs
            bp.predict_to_dir(files[:batch], outs[k])
        got = {k: [] for k in preds}
        for _ in range(repeats):
            for k, bp in preds.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                bp.predict_to_dir(files, outs[k])
                torch.cuda.synchronize()
                got[k].append(n_images / (time.perf_counter() - t0))
        return {k: (statistics.median(v), min(v), max(v)) for k, v in got.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="a,b,c")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--folder-repeats", type=int, default=3)
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("fullframe_bench needs an AMD GPU: a timing taken anywhere else says nothing")
    legs = args.legs.split(",")
    lines = ["# Full-frame pre/post-processing: measured", "",
             f"`python tools/fullframe_bench.py` on {torch.cuda.get_device_name(0)}, 16 host CPUs; clocks after the run: {{clock}}.", ""]

    def fmt(t):
        return f"{t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f})"

    if "a" in legs:
        lines += [f"## (a) Post: {B} maps of {NET[0]}x{NET[1]} -> {B} outputs of the originals' size", "",
                  f"Median of {args.repeats} alternating windows between HIP events (min .. max), ms per batch of {B}.  `torch loop` = "
                  "per image F.interpolate, clamp, (normalize,) quantise / colormap into a preallocated output.", "",
                  "| mode | output | one call | torch loop | loop / call | output GB/s (call) | call faster |", "|---|---|---|---|---|---|---|"]
        for r in leg_a(args.repeats):
            k, l = r["kernel"], r["loop"]
            lines.append(f"| {r['mode']} | {r['shape']} | {fmt(k)} | {fmt(l)} | {l[0] / k[0]:.2f}x | {r['bytes'] / (k[0] * 1e-3) / 1e9:.0f} | "
                         f"{'yes' if k[0] < l[0] else 'NO'} |")
            print(lines[-1], flush=True)
        lines.append("")
    if "b" in legs:
        lines += [f"## (b) Pre: {B} device-resident RGB images -> x [{B},3,{NET[0]},{NET[1]}]", "",
                  f"Median of {args.repeats} windows between HIP events (min .. max), ms per batch of {B}; the PIL column is {B} x the mean "
                  "of 4 host resizes + ToTensor on one core, for reference only (another device, another clock).", "",
                  "| input | one call | input GB/s | PIL on the host (reference only) |", "|---|---|---|---|"]
        for r in leg_b(args.repeats):
            k = r["kernel"]
            lines.append(f"| {r['shape']} | {fmt(k)} | {r['bytes'] / (k[0] * 1e-3) / 1e9:.0f} | {r['pil_ms']:.0f} |")
            print(lines[-1], flush=True)
        lines.append("")
    if "c" in legs:
        t = leg_c(args.images, args.folder_repeats)
        lines += [f"## (c) A folder of {args.images} PNGs (512x640 RGB), task `normal`, bf16, batch_size 32", "",
                  f"Images per second through `predict_to_dir`, median of {args.folder_repeats} alternating runs (min .. max); host clock around "
                  "runs that end in a device synchronise.  `None` writes 384x384 maps and 512x512 previews; the full-frame modes write "
                  "512x640 maps and the unchanged image (network 384x384 for squash, 384x480 for aspect).", "",
                  "| full_frame | images / s |", "|---|---|"]
        for k in ("None", "squash", "aspect"):
            lines.append(f"| {k} | {t[k][0]:.1f} ({t[k][1]:.1f} .. {t[k][2]:.1f}) |")
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
