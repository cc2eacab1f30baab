"""Times the blend of tiled inference (dptx_tile_blend_normals; dptx_tile_align_depth + dptx_tile_blend_depth) against the same
blend composed from torch fp32 ops on the same GPU, and TiledNormals / TiledDepth end to end against the plain forwards of the
same tiles.

    python tools/tiled_bench.py [--legs a,b] [--repeats 5] [--out profiles/tiled_bench.md]

(a) the blend alone: a 4000x3000 image, plan_tiles' 14 x 11 tiles of 384x384 (window = network size, ramps of 96), random maps in
    [0, 1] (depth: a smooth field seen through a random scale and shift per tile, plus noise; the anchor at 384x512).
    `one call` = dptx_tile_blend_normals into a preallocated uint8 output; for depth dptx_tile_align_depth then
    dptx_tile_blend_depth into preallocated coefficients, workspace and fp32 output.
    `torch` = per tile decode / clamp (+ F.normalize) and F.interpolate into the window, the weight plane of the tile (outer product
    of the two axis ramps), an indexed accumulate into [C,H,W] (and the weight sum), then the normalisation, clamp and * 255 ->
    uint8 HWC; for depth first the anchor resized to the image, per tile the four sums over its window and the 2 x 2 solve on the
    device (nothing read back).  Windows between HIP events, at least 50 ms each, the two paths alternating; median (min .. max).
(b) end to end: TiledNormals / TiledDepth (batch_size 32) on one 4000x3000 RGB image (bf16 DPT-Hybrid, random weights) against
    `forwards`: model(x) on preallocated inputs of the same tiles (and the anchor) in the same batches -- what the network alone
    costs.  Host clock around runs that end in a device synchronise; runs alternate.
"""
from __future__ import annotations

import argparse
import ctypes as C
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

SIZE = (3000, 4000)   # (H, W)


def _axis_weights(starts, c, r, L, dev):
    t = torch.arange(c, device=dev, dtype=torch.float32)
    one = torch.ones(c, device=dev)
    res = []
    for s in starts:
        left = one if (s == 0 or r == 0) else torch.minimum(one, (t + 0.5) / r)
        right = one if (s + c == L or r == 0) else torch.minimum(one, ((c - 1 - t) + 0.5) / r)
        res.append(left * right)
    return res


def torch_blend_normals(maps, plan, out):
    """maps [tiles,3,h,w] -> out [H,W,3] uint8: what a user would write around F.interpolate."""
    H, W = SIZE
    (ch, cw), (ry, rx) = plan.window, plan.ramps
    wy, wx = _axis_weights(plan.ys, ch, ry, H, out.device), _axis_weights(plan.xs, cw, rx, W, out.device)
    acc = torch.zeros(3, H, W, device=out.device)
    for iy, y0 in enumerate(plan.ys):
        for ix, x0 in enumerate(plan.xs):
            n = F.normalize(2 * maps[iy * len(plan.xs) + ix] - 1, dim=0, eps=1e-12)
            v = F.interpolate(n[None], (ch, cw), mode="bilinear", align_corners=False)[0]
            acc[:, y0:y0 + ch, x0:x0 + cw] += (wy[iy][:, None] * wx[ix][None, :]) * v
    out.copy_((((F.normalize(acc, dim=0, eps=1e-12) + 1) / 2).clamp(0, 1) * 255).to(torch.uint8).permute(1, 2, 0))


def torch_align_blend_depth(maps, anchor, plan, out):
    """maps [tiles,h,w], anchor [ah,aw] -> out [H,W] fp32"""
    H, W = SIZE
    (ch, cw), (ry, rx) = plan.window, plan.ramps
    wy, wx = _axis_weights(plan.ys, ch, ry, H, out.device), _axis_weights(plan.xs, cw, rx, W, out.device)
    a_full = F.interpolate(anchor.clamp(0, 1)[None, None], (H, W), mode="bilinear", align_corners=False)[0, 0]
    acc, wsum = torch.zeros(H, W, device=out.device), torch.zeros(H, W, device=out.device)
    n = float(ch * cw)
    for iy, y0 in enumerate(plan.ys):
        for ix, x0 in enumerate(plan.xs):
            r = F.interpolate(maps[iy * len(plan.xs) + ix].clamp(0, 1)[None, None], (ch, cw), mode="bilinear", align_corners=False)[0, 0]
            a = a_full[y0:y0 + ch, x0:x0 + cw]
            sr, srr, sa, sra = r.sum(), (r * r).sum(), a.sum(), (r * a).sum()
            det = n * srr - sr * sr
            ok = det > 1e-10 * n * srr
            safe = torch.where(ok, det, torch.ones_like(det))
            s = torch.where(ok, (n * sra - sr * sa) / safe, torch.ones_like(det))
            t = torch.where(ok, (srr * sa - sr * sra) / safe, (sa - sr) / n)
            w = wy[iy][:, None] * wx[ix][None, :]
            acc[y0:y0 + ch, x0:x0 + cw] += w * (s * r + t)
            wsum[y0:y0 + ch, x0:x0 + cw] += w
    out.copy_(1 - (acc / wsum).clamp(0, 1))


def leg_a(repeats):
    from omnidata_amd import preprocess as pp
    from omnidata_amd.engine import load_library
    from omnidata_amd.tiled import plan_tiles
    lib = load_library()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    H, W = SIZE
    plan = plan_tiles(W, H)
    n_tiles, (h, w), (ah, aw) = len(plan.ys) * len(plan.xs), plan.net, plan.anchor_net
    g = torch.Generator(device="cuda").manual_seed(0)
    rows = []

    # ---- normals, uint8
    maps = torch.rand(n_tiles, 3, h, w, device=dev, generator=g)
    grid = (pp.TileGrid * 1)(pp.TileGrid.make(0, plan.net, plan.window, plan.ys, plan.xs, plan.ramps))
    descs, total = pp.output_layout([SIZE], "normal_u8")
    out = torch.empty(total, dtype=torch.uint8, device=dev)
    ref = torch.empty(H, W, 3, dtype=torch.uint8, device=dev)

    def kernel():
        assert lib.dptx_tile_blend_normals(maps.data_ptr(), C.addressof(grid), C.addressof(descs), 1, 1, out.data_ptr(), stream) == 0

    def loop():
        torch_blend_normals(maps, plan, ref)

    kernel()
    loop()
    torch.cuda.synchronize()
    d = (out[:3 * H * W].view(H, W, 3).to(torch.int16) - ref.to(torch.int16)).abs()
    t = alternate(dict(kernel=kernel, loop=loop), repeats)
    rows.append(dict(what="normals uint8", tiles=n_tiles, map_bytes=maps.numel() * 4, kernel=t["kernel"], loop=t["loop"],
                     diff=f"{int(d.max())} level(s), {float((d > 0).float().mean()):.1e} of bytes"))
    del maps, out, ref
    torch.cuda.empty_cache()

    # ---- depth, fp32, with the alignment
    ys = (torch.arange(H, device=dev) + 0.5) / H
    xs = (torch.arange(W, device=dev) + 0.5) / W
    truth = 0.5 + 0.2 * torch.sin(4 * xs[None, :] + ys[:, None]) * torch.cos(3 * ys[:, None] - 2 * xs[None, :])
    flat = torch.empty(n_tiles * h * w + ah * aw, device=dev)
    maps = flat[:n_tiles * h * w].view(n_tiles, h, w)
    for k in range(n_tiles):
        y0, x0 = plan.ys[k // len(plan.xs)], plan.xs[k % len(plan.xs)]
        a, b = 0.8 + 0.45 * float(torch.rand(1, device=dev, generator=g)), -0.05 + 0.1 * float(torch.rand(1, device=dev, generator=g))
        maps[k] = (truth[y0:y0 + h, x0:x0 + w] - b) / a + 0.01 * torch.randn(h, w, device=dev, generator=g)
    anchor = flat[n_tiles * h * w:].view(ah, aw)
    anchor.copy_(F.interpolate(truth[None, None], (ah, aw), mode="bilinear", align_corners=False, antialias=True)[0, 0])
    grid = (pp.TileGrid * 1)(pp.TileGrid.make(0, plan.net, plan.window, plan.ys, plan.xs, plan.ramps, 4 * n_tiles * h * w, (ah, aw)))
    descs, total = pp.output_layout([SIZE], "depth_f32")
    nbytes = C.c_int64()
    assert lib.dptx_tile_depth_workspace_bytes(C.addressof(grid), C.addressof(descs), 1, C.byref(nbytes)) == 0
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    coeffs = torch.empty(n_tiles, 2, device=dev)
    out = torch.empty(total, dtype=torch.uint8, device=dev)
    ref = torch.empty(H, W, device=dev)

    def kernel_d():
        assert lib.dptx_tile_align_depth(flat.data_ptr(), C.addressof(grid), C.addressof(descs), 1, coeffs.data_ptr(), ws.data_ptr(),
                                         ws.numel(), stream) == 0
        assert lib.dptx_tile_blend_depth(flat.data_ptr(), C.addressof(grid), coeffs.data_ptr(), C.addressof(descs), 1, 3, out.data_ptr(),
                                         stream) == 0

    def loop_d():
        torch_align_blend_depth(maps, anchor, plan, ref)

    kernel_d()
    loop_d()
    torch.cuda.synchronize()
    diff = float((out[:4 * H * W].view(torch.float32).view(H, W) - ref).abs().max())
    t = alternate(dict(kernel=kernel_d, loop=loop_d), repeats)
    rows.append(dict(what="depth fp32, aligned", tiles=n_tiles, map_bytes=flat.numel() * 4, kernel=t["kernel"], loop=t["loop"],
                     diff=f"{diff:.1e}"))
    return rows


def leg_b(repeats):
    from omnidata_amd.model import build_model
    from omnidata_amd.tiled import TiledDepth, TiledNormals, plan_tiles
    dev = torch.device("cuda:0")
    H, W = SIZE
    plan = plan_tiles(W, H)
    n_tiles = len(plan.ys) * len(plan.xs)
    img = Image.fromarray(np.random.default_rng(0).integers(0, 256, (H, W, 3), dtype=np.uint8))
    rows = []
    for task in ("normal", "depth"):
        model = build_model(task, random_weights=0, dtype="bf16", max_batch=32).to(dev)
        run = (TiledDepth if task == "depth" else TiledNormals)(model, batch_size=32)
        xs = [torch.rand(1, 3, *plan.anchor_net, device=dev)] if task == "depth" else []
        xs += [torch.rand(min(32, n_tiles - b0), 3, *plan.net, device=dev) for b0 in range(0, n_tiles, 32)]

        def end_to_end():
            run([img])

        def forwards():
            with torch.no_grad():
                for x in xs:
                    model(x)

        got = {"end_to_end": [], "forwards": []}
        for fn in (end_to_end, forwards):
            fn()
        torch.cuda.synchronize()
        for _ in range(repeats):
            for name, fn in (("end_to_end", end_to_end), ("forwards", forwards)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                got[name].append((time.perf_counter() - t0) * 1e3)
        rows.append(dict(task=task, forwards_n=len(xs), tiles=n_tiles,
                         **{k: (statistics.median(v), min(v), max(v)) for k, v in got.items()}))
        del model, run, xs
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="a,b")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("tiled_bench needs an AMD GPU: a timing taken anywhere else says nothing")
    legs = args.legs.split(",")
    lines = ["# Tiled inference: measured", "",
             f"`python tools/tiled_bench.py` on {torch.cuda.get_device_name(0)}, 16 host CPUs; clocks after the run: {{clock}}.", ""]

    def fmt(t):
        return f"{t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f})"

    if "a" in legs:
        lines += [f"## (a) The blend alone: 14 x 11 tiles of 384x384 -> one {SIZE[1]}x{SIZE[0]} map", "",
                  f"Median of {args.repeats} alternating windows between HIP events (min .. max), ms per call.  `one call` = "
                  "`dptx_tile_blend_normals` (uint8 output), or `dptx_tile_align_depth` + `dptx_tile_blend_depth` (fp32 output); `torch` = "
                  "per tile decode / clamp, F.interpolate, the tile's weight plane and an indexed accumulate, for depth with the anchor "
                  "resized once and 154 sets of four fp32 sums and solves on the device.  `difference` = the largest difference between "
                  "the two results (the torch path sums in fp32; tests/test_gpu_tiled.py holds the parity check).", "",
                  "| output | tiles | tile maps MB | one call | torch | torch / call | difference | call faster |",
                  "|---|---|---|---|---|---|---|---|"]
        for r in leg_a(args.repeats):
            k, l = r["kernel"], r["loop"]
            lines.append(f"| {r['what']} | {r['tiles']} | {r['map_bytes'] / 1e6:.0f} | {fmt(k)} | {fmt(l)} | {l[0] / k[0]:.1f}x | "
                         f"{r['diff']} | {'yes' if k[0] < l[0] else 'NO'} |")
            print(lines[-1], flush=True)
        lines.append("")
    if "b" in legs:
        lines += [f"## (b) End to end: one {SIZE[1]}x{SIZE[0]} RGB image, tile 384, scale 1.0, overlap 0.25, batch_size 32, bf16 DPT-Hybrid", "",
                  f"Median of {args.repeats} alternating runs (min .. max), ms per call; host clock around runs that end in a device "
                  "synchronise.  `forwards` = model(x) alone on preallocated inputs of the same tiles (depth: and the anchor) in the same "
                  "batches; `pre + blend share` = (end to end - forwards) / end to end: upload, tile inputs, the copies of the maps, "
                  "alignment, blend, colouring.", "",
                  "| task | tiles | forwards per call | end to end | forwards | pre + blend share |", "|---|---|---|---|---|---|"]
        for r in leg_b(args.repeats):
            e, f = r["end_to_end"], r["forwards"]
            lines.append(f"| {r['task']} | {r['tiles']} | {r['forwards_n']} | {fmt(e)} | {fmt(f)} | {100 * (e[0] - f[0]) / e[0]:.1f} % |")
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
