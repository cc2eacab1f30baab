"""Times guided upsampling (dptx_postprocess_guided_batch) against the plain resize it replaces and against the same filter composed
from torch ops on the same GPU, and a folder of PNGs through BatchPredictor.predict_to_dir with and without `guided`.

    python tools/guided_bench.py [--legs a,b] [--repeats 5] [--folder-repeats 3] [--images 256] [--radius 2] [--out profiles/guided_bench.md]

(a) 32 maps of 384x512 -> 32 outputs of 512x640, 1080x1920 and 3000x4000 in the four output modes: one guided call, one
    dptx_postprocess_resize_batch call on the same maps and output buffer, and -- for ONE image, scaled to 32 in the table -- the
    filter composed from torch fp32 ops (per tap a gather of the guide and the map, an exponent, a running minimum; then the
    weights and sums; clamp and quantisation).  Windows between HIP events, at least 50 ms each, the paths alternating; the
    figure is the median, min..max its spread.  Behind the table, what bounds the kernel: the time its VALU instructions, its LDS
    traffic and its memory traffic would each take alone at the device's peak rates, next to the measured time.
(b) a folder of PNGs (512x640) written at run time: predict_to_dir with full_frame="aspect", with and without guided=True,
    batch_size 32, bf16.  Host clock around runs that end in a device synchronise; runs alternate.
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

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from batch_infer_bench import alternate, clock_note, make_folder  # noqa: E402

SHAPES = [(512, 640), (1080, 1920), (3000, 4000)]
NET = (384, 512)
B = 32
SIGMA_SPACE, SIGMA_RANGE = 1.0, 0.1
# device peaks the bound estimates use (MI355X: 256 CUs of 4 SIMDs at 2.4 GHz; a SIMD issues a wave64 VALU instruction over 2
# cycles and a transcendental over 8; 128 bytes of LDS per CU and clock; 8 TB/s of HBM)
CUS, CLOCK_HZ, LDS_BYTES_PER_CLK, HBM_BYTES_PER_S = 256, 2.4e9, 128, 8.0e12
VALU_CYCLES, TRANS_CYCLES = 2, 8
# (plain VALU, transcendental) instructions per output pixel, keyed by (radius, map channels), counted in the compiled code
# (hipcc -S on csrc/guided.hip, guided_kernel<R, NORMAL_U8> and <R, DEPTH_F32>): the basic block of the staged pixel body plus the
# per-pixel prologue in front of it (coordinates, the guide pixel's three divisions, the clamped tap offsets)
VALU_PER_PIXEL = {(1, 3): (313, 10), (2, 3): (761, 22), (3, 3): (1493, 42), (1, 1): (272, 8), (2, 1): (672, 20), (3, 1): (1324, 40)}


def torch_guided(S, G_lo, pixels, radius, mode, renorm=False, lut=None):
    """The definition of include/dptx.h ("Guided upsampling") in torch fp32 ops on the tensors' device, one image:
    S [C,h,w], G_lo [3,h,w], pixels [H,W,3] uint8 -> the mode's output."""
    Cn, h, w = S.shape
    H, W = pixels.shape[:2]
    dev = S.device
    gh = pixels.permute(2, 0, 1).float() / 255
    ks, kr = 1.0 / (2 * SIGMA_SPACE ** 2), 1.0 / (2 * SIGMA_RANGE ** 2)
    sy = (h / H) * (torch.arange(H, device=dev, dtype=torch.float32) + 0.5) - 0.5
    sx = (w / W) * (torch.arange(W, device=dev, dtype=torch.float32) + 0.5) - 0.5
    by, bx = sy.floor().long(), sx.floor().long()
    exps, taps = [], []
    for j in range(2 * radius):
        qy = by - radius + 1 + j
        oky, qyc = (qy >= 0) & (qy < h), qy.clamp(0, h - 1)
        dy2 = (qy.float() - sy) ** 2
        for i in range(2 * radius):
            qx = bx - radius + 1 + i
            okx, qxc = (qx >= 0) & (qx < w), qx.clamp(0, w - 1)
            dx2 = (qx.float() - sx) ** 2
            diff = gh - G_lo[:, qyc][:, :, qxc]
            e = ks * (dy2[:, None] + dx2[None, :]) + kr * (diff * diff).sum(0)
            e = e.masked_fill(~(oky[:, None] & okx[None, :]), float("inf"))
            exps.append(e)
            taps.append((qyc, qxc))
    emin = exps[0]
    for e in exps[1:]:
        emin = torch.minimum(emin, e)
    den = torch.zeros(H, W, device=dev)
    acc = torch.zeros(Cn, H, W, device=dev)
    for e, (qyc, qxc) in zip(exps, taps):
        wgt = torch.exp(emin - e)
        den += wgt
        acc += wgt[None] * S[:, qyc][:, :, qxc]
    v = acc / den
    if mode.startswith("normal"):
        if renorm:
            v = (torch.nn.functional.normalize(2 * v - 1, dim=0) + 1) / 2
        v = v.clamp(0, 1)
        return v if mode == "normal_f32" else v.mul(255).byte().permute(1, 2, 0).contiguous()
    d = 1 - v[0].clamp(0, 1)
    if mode == "depth_f32":
        return d
    lo, hi = d.min(), d.max()
    return lut.view(256, 4)[((d - lo) / (hi - lo) * 256).clamp(0, 255).long()]


def leg_a(repeats, radius):
    from omnidata_amd import preprocess as pp
    from omnidata_amd._native import workspace
    from omnidata_amd.engine import load_library
    lib = load_library()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    lut = torch.from_numpy(pp.viridis_lut()).to(dev)
    params = pp.GuidedParams(radius, SIGMA_SPACE, SIGMA_RANGE)
    ws = workspace("dptx_postprocess_guided_workspace_bytes", dev, (B, 4), "unsupported")
    rows = []
    for H, W in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(H)
        # a smooth low-resolution colour field and its bilinear resize with noise as the image: the guides agree as a photo and its
        # network input do
        G_lo = torch.rand(B, 3, NET[0] // 16, NET[1] // 16, device=dev, generator=g)
        G_lo = torch.nn.functional.interpolate(G_lo, NET, mode="bicubic", align_corners=False).clamp(0, 1).contiguous()
        one = (H * W * 3 + 15) // 16 * 16
        pixels = torch.empty(B * one, dtype=torch.uint8, device=dev)
        for i in range(B):
            hi = torch.nn.functional.interpolate(G_lo[i:i + 1], (H, W), mode="bilinear", align_corners=False)[0]
            hi = (hi + 0.02 * torch.randn(3, H, W, device=dev, generator=g)).clamp(0, 1)
            pixels[i * one:i * one + H * W * 3] = hi.mul(255).byte().permute(1, 2, 0).reshape(-1)
            del hi
        guides = (pp.ImageDesc * B)(*[pp.ImageDesc(i * one, H, W, 3, W * 3) for i in range(B)])
        for mode, code, Cn in (("normal_u8", 1, 3), ("normal_f32", 2, 3), ("depth_f32", 3, 1), ("depth_rgba", 4, 1)):
            y = torch.rand(B, Cn, *NET, device=dev, generator=g)
            descs, total = pp.output_layout([(H, W)] * B, mode)
            out = torch.empty(total, dtype=torch.uint8, device=dev)

            def guided():
                assert lib.dptx_postprocess_guided_batch(y.data_ptr(), G_lo.data_ptr(), B, Cn, NET[0], NET[1], pixels.data_ptr(),
                                                         C.addressof(guides), C.addressof(descs), C.addressof(params), code,
                                                         out.data_ptr(), lut.data_ptr(), ws.data_ptr(), ws.numel(), stream) == 0

            def resize():
                assert lib.dptx_postprocess_resize_batch(y.data_ptr(), B, Cn, NET[0], NET[1], C.addressof(descs), code, out.data_ptr(),
                                                         lut.data_ptr(), ws.data_ptr(), ws.numel(), stream) == 0

            img = pixels[:H * W * 3].view(H, W, 3)

            def composed():   # one image
                torch_guided(y[0], G_lo[0], img, radius, mode, lut=lut)

            t = alternate(dict(guided=guided, resize=resize, composed=composed), repeats)
            rows.append(dict(mode=mode, shape=f"{H}x{W}", pixels=B * H * W, out_bytes=total, Cn=Cn, **t))
            del out, y
            torch.cuda.empty_cache()
        del pixels, G_lo
        torch.cuda.empty_cache()
    return rows


def leg_b(n_images, repeats, batch=32):
    from omnidata_amd.batch_infer import BatchPredictor
    from omnidata_amd.model import build_model
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "in")
        os.makedirs(src)
        make_folder(src, n_images)
        files = sorted(glob.glob(src + "/*"))
        model = build_model("normal", random_weights=0, dtype="bf16", max_batch=batch).to("cuda:0")
        preds = {"plain": BatchPredictor(model, "normal", batch_size=batch, full_frame="aspect"),
                 "guided": BatchPredictor(model, "normal", batch_size=batch, full_frame="aspect", guided=True)}
        outs = {k: os.path.join(tmp, k) for k in preds}
        for k, bp in preds.items():
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


def bounds_ms(pixels, Cn, radius, out_bytes):
    """-> (VALU, LDS, memory) ms: what each would take alone at the device's peak rate."""
    valu, trans = VALU_PER_PIXEL[(radius, Cn)]
    taps = 4 * radius * radius
    valu_ms = pixels * (valu * VALU_CYCLES + trans * TRANS_CYCLES) / 64 / (CUS * 4 * CLOCK_HZ) * 1e3   # SIMD cycles per wave / 64 lanes
    lds_ms = pixels * taps * (16 + 4 * Cn) / (CUS * LDS_BYTES_PER_CLK * CLOCK_HZ) * 1e3
    mem_ms = (out_bytes + pixels * 3) / HBM_BYTES_PER_S * 1e3
    return valu_ms, lds_ms, mem_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="a,b")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--folder-repeats", type=int, default=3)
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--radius", type=int, default=2, choices=[1, 2, 3])
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("guided_bench needs an AMD GPU: a timing taken anywhere else says nothing")
    legs = args.legs.split(",")
    lines = ["# Guided upsampling: measured", "",
             f"`python tools/guided_bench.py` on {torch.cuda.get_device_name(0)}, 16 host CPUs; clocks after the run: {{clock}}.", ""]

    def fmt(t):
        return f"{t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f})"

    if "a" in legs:
        rows = leg_a(args.repeats, args.radius)
        lines += [f"## (a) {B} maps of {NET[0]}x{NET[1]} -> {B} outputs, radius {args.radius}, sigma_space {SIGMA_SPACE}, sigma_range {SIGMA_RANGE}", "",
                  f"Median of {args.repeats} alternating windows between HIP events (min .. max), ms per batch of {B}.  `plain resize` = "
                  "`dptx_postprocess_resize_batch` on the same maps into the same buffer; `torch ops` = the filter composed from torch fp32 "
                  f"ops, timed on ONE image and multiplied by {B}.", "",
                  "| mode | output | guided call | plain resize | guided / plain | torch ops (x32) | torch / guided | Gpixel/s (guided) |",
                  "|---|---|---|---|---|---|---|---|"]
        for r in rows:
            g, p, c = r["guided"], r["resize"], r["composed"]
            lines.append(f"| {r['mode']} | {r['shape']} | {fmt(g)} | {fmt(p)} | {g[0] / p[0]:.1f}x | {c[0] * B:.0f} | {c[0] * B / g[0]:.0f}x | "
                         f"{r['pixels'] / (g[0] * 1e-3) / 1e9:.1f} |")
            print(lines[-1], flush=True)
        lines += ["", "What bounds the kernel: the time each resource would take alone at its peak rate (256 CUs of 4 SIMDs at 2.4 GHz; 2 cycles per "
                  "wave64 VALU instruction and 8 per transcendental, counted per pixel in the compiled kernel; 128 B of LDS per CU "
                  "and clock; 8 TB/s of HBM for the output and the guide pixels), next to the measured time.", "",
                  "| mode | output | measured | VALU alone | LDS alone | memory alone |", "|---|---|---|---|---|---|"]
        for r in rows:
            v, l, m = bounds_ms(r["pixels"], r["Cn"], args.radius, r["out_bytes"])
            lines.append(f"| {r['mode']} | {r['shape']} | {r['guided'][0]:.3f} | {v:.3f} | {l:.3f} | {m:.3f} |")
            print(lines[-1], flush=True)
        lines.append("")
    if "b" in legs:
        t = leg_b(args.images, args.folder_repeats)
        lines += [f"## (b) A folder of {args.images} PNGs (512x640 RGB), task `normal`, bf16, batch_size 32, full_frame=\"aspect\"", "",
                  f"Images per second through `predict_to_dir`, median of {args.folder_repeats} alternating runs (min .. max); host clock "
                  "around runs that end in a device synchronise.  Both write 512x640 maps and the unchanged image (network 384x480).", "",
                  "| last step | images / s |", "|---|---|"]
        for k, name in (("plain", "plain resize (guided=None)"), ("guided", "guided=True")):
            lines.append(f"| {name} | {t[k][0]:.1f} ({t[k][1]:.1f} .. {t[k][2]:.1f}) |")
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
