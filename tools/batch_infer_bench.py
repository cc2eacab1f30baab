"""Times image ingestion for a batch: the ragged-batch pre-processing against the single-image entry, and a folder of PNGs
through omnidata_amd.batch_infer against demo.py's per-image loop.

    python tools/batch_infer_bench.py [--legs a,b] [--repeats 5] [--folder-repeats 3] [--images 256] [--out profiles/batch_infer_bench.md]

(a) pre-processing alone, B = 32 device-resident images: one dptx_preprocess_u8_batch call against 32 dptx_preprocess_u8
    calls (whose first call per size, which allocates and copies its table, is made before the windows), at 512x640,
    1080x1920, 3000x4000 and a mix of the three.  Windows between HIP events, at least 50 ms each, the two paths
    alternating; the figure is the median, min..max its spread.  The outputs of the two paths are compared first.
(b) a folder of PNGs written at run time into a temporary directory: the per-image loop of demo.py (max_batch=1: open,
    upload, pre, forward, post, blocking read-back, PNG) against BatchPredictor.predict_to_dir at batch_size=32, and the batched
    path once more on decoded arrays with the outputs left on the device, for `normal` in `mixed` and `bf16`.  Host clock
    around work that ends in a device synchronise; runs alternate.
"""
from __future__ import annotations

import argparse
import ctypes as C
import glob
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {"512x640": [(512, 640)], "1080x1920": [(1080, 1920)], "3000x4000": [(3000, 4000)],
         "mixed": [(512, 640), (1080, 1920), (3000, 4000)]}


def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def alternate(fns: dict, repeats, min_window_ms=50.0):
    calls = {}
    for name, fn in fns.items():
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        calls[name] = max(2, int(min_window_ms / max(window(fn, 2), 1e-4)) + 1)
    got = {name: [] for name in fns}
    for _ in range(repeats):
        for name, fn in fns.items():
            got[name].append(window(fn, calls[name]))
    return {name: (statistics.median(v), min(v), max(v)) for name, v in got.items()}


def leg_a(repeats, B=32, S=384):
    from omnidata_amd import preprocess as pp
    from omnidata_amd._native import workspace
    from omnidata_amd.engine import load_library
    lib = load_library()
    dev = torch.device("cuda:0")
    rows = []
    for name, shapes in SIZES.items():
        g = torch.Generator(device="cuda").manual_seed(len(name))
        imgs = [torch.randint(0, 256, (*shapes[i % len(shapes)], 3), dtype=torch.uint8, device=dev, generator=g) for i in range(B)]
        offs, off = [], 0
        for t in imgs:
            offs.append(off)
            off = (off + t.numel() + 15) // 16 * 16
        packed = torch.empty(off, dtype=torch.uint8, device=dev)
        descs = (pp.ImageDesc * B)()
        for i, (t, o) in enumerate(zip(imgs, offs)):
            packed[o:o + t.numel()] = t.reshape(-1)
            descs[i] = pp.ImageDesc(o, t.shape[0], t.shape[1], 3, t.shape[1] * 3)
        ws = workspace("dptx_preprocess_batch_workspace_bytes", dev, (B, S), "unsupported")
        xb = torch.empty(B, 3, S, S, device=dev)
        xs = torch.empty(B, 3, S, S, device=dev)
        stream = torch.cuda.current_stream().cuda_stream

        def batched():
            assert lib.dptx_preprocess_u8_batch(packed.data_ptr(), C.addressof(descs), B, S, 0, xb.data_ptr(), ws.data_ptr(),
                                                ws.numel(), stream) == 0

        calls = [(t.data_ptr(), t.shape[0], t.shape[1], 3, t.shape[1] * 3, 0, xs[i].data_ptr(), stream) for i, t in enumerate(imgs)]

        def single():
            for c in calls:
                assert lib.dptx_preprocess_u8(*c) == 0

        single()   # the first call per size allocates its table: outside the windows
        batched()
        torch.cuda.synchronize()
        same = bool(torch.equal(xb, xs))
        t = alternate(dict(batched=batched, single=single), repeats)
        nbytes = sum(x.numel() for x in imgs)
        rows.append(dict(name=name, same=same, bytes=nbytes, batched=t["batched"], single=t["single"]))
        del imgs, packed
        torch.cuda.empty_cache()
    return rows


def make_folder(path, n, seed=0):
    """n RGB PNGs of 512x640: smooth fields plus a little noise (a photograph's PNG, not a noise image's)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:512, 0:640].astype(np.float32)
    for i in range(n):
        f = rng.uniform(0.005, 0.03, size=(3, 2))
        ph = rng.uniform(0, 6.28, size=3)
        img = np.stack([127 + 100 * np.sin(f[c, 0] * yy + f[c, 1] * xx + ph[c]) for c in range(3)], -1)
        img += rng.normal(0, 4, img.shape)
        Image.fromarray(img.clip(0, 255).astype(np.uint8)).save(os.path.join(path, f"img{i:04d}.png"))


def per_image_loop(model, files, out_dir, task="normal"):
    """demo.py's loop over a directory (its save_outputs, statement for statement, without the prints)."""
    from omnidata_amd import preprocess as pp
    device = torch.device("cuda:0")
    with torch.no_grad():
        for f in files:
            stem = os.path.splitext(os.path.basename(f))[0]
            save_path = os.path.join(out_dir, f"{stem}_{task}.png")
            img = Image.open(f)
            img_tensor = pp.image_to_input_gpu(img, task, device)
            pp.rgb_preview(img).save(os.path.join(out_dir, f"{stem}_rgb.png"))
            output = model(img_tensor).clamp(min=0, max=1)
            Image.fromarray(pp.normal_to_u8_gpu(output[0]).cpu().numpy()).save(save_path)


def leg_b(n_images, repeats, batch=32):
    from omnidata_amd.batch_infer import BatchPredictor
    from omnidata_amd.model import build_model
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "in")
        os.makedirs(src)
        make_folder(src, n_images)
        files = sorted(glob.glob(src + "/*"))
        arrays = [np.asarray(Image.open(f)) for f in files]
        for dtype in ("mixed", "bf16"):
            m1 = build_model("normal", random_weights=0, dtype=dtype, max_batch=1).to("cuda:0")
            mb = build_model("normal", random_weights=0, dtype=dtype, max_batch=batch).to("cuda:0")
            bp = BatchPredictor(mb, "normal", batch_size=batch)
            outs = [os.path.join(tmp, f"{dtype}_{k}") for k in ("loop", "batch")]
            for o in outs:
                os.makedirs(o)

            def run_loop():
                per_image_loop(m1, files, outs[0])

            def run_batch():
                bp.predict_to_dir(files, outs[1])

            def run_gpu_only():
                for _ in bp.predict(arrays):
                    pass

            warm = files[:batch]
            per_image_loop(m1, warm[:4], outs[0])
            bp.predict_to_dir(warm, outs[1])
            got = {"loop": [], "batch": [], "gpu_only": []}
            for _ in range(repeats):
                for name, fn in (("loop", run_loop), ("batch", run_batch), ("gpu_only", run_gpu_only)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    got[name].append(n_images / (time.perf_counter() - t0))
            same = all(np.array_equal(np.asarray(Image.open(os.path.join(outs[0], n))), np.asarray(Image.open(os.path.join(outs[1], n))))
                       for n in sorted(os.listdir(outs[0]))[:16])
            rows.append(dict(dtype=dtype, same=same, **{k: (statistics.median(v), min(v), max(v)) for k, v in got.items()}))
            del m1, mb, bp
            torch.cuda.empty_cache()
    return rows


def clock_note():
    try:
        r = subprocess.run(["/opt/rocm/bin/rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30)
        lines = [l.strip() for l in r.stdout.splitlines() if "GPU[0]" in l and ("sclk" in l or "mclk" in l)]
        return "; ".join(lines) if lines else "not read"
    except Exception:  # noqa: BLE001
        return "not read"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="a,b")
    ap.add_argument("--repeats", type=int, default=5, help="windows per path in (a)")
    ap.add_argument("--folder-repeats", type=int, default=3, help="runs per path in (b)")
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("batch_infer_bench needs an AMD GPU: a timing taken anywhere else says nothing")
    lines = ["# Batched image ingestion: measured", "",
             f"`python tools/batch_infer_bench.py` on {torch.cuda.get_device_name(0)}, 16 host CPUs; clocks after the run: {{clock}}.", ""]
    legs = args.legs.split(",")
    if "a" in legs:
        lines += ["## (a) Pre-processing alone, B = 32, S = 384, device-resident RGB images", "",
                  f"Median of {args.repeats} alternating windows between HIP events (min .. max), ms per batch of 32.", "",
                  "| input | batched call | 32 single calls | single / batched | input GB/s (batched) | same bits | batched not slower |",
                  "|---|---|---|---|---|---|---|"]
        for r in leg_a(args.repeats):
            b, s = r["batched"], r["single"]
            verdict = "yes" if b[0] <= s[0] or b[1] <= s[2] else "NO"
            lines.append(f"| {r['name']} | {b[0]:.3f} ({b[1]:.3f} .. {b[2]:.3f}) | {s[0]:.3f} ({s[1]:.3f} .. {s[2]:.3f}) | {s[0] / b[0]:.2f}x | "
                         f"{r['bytes'] / (b[0] * 1e-3) / 1e9:.0f} | {'yes' if r['same'] else 'NO'} | {verdict} |")
            print(lines[-1], flush=True)
        lines.append("")
    if "b" in legs:
        lines += [f"## (b) A folder of {args.images} PNGs (512x640 RGB), task `normal`", "",
                  f"Images per second, median of {args.folder_repeats} alternating runs (min .. max); host clock around runs that end in a "
                  "device synchronise.  `batched` = `predict_to_dir`, batch_size 32, 8 workers; `GPU side` = `predict` on decoded arrays, "
                  "outputs left on the device (no PNG codec).", "",
                  "| dtype | per-image loop | batched | batched / loop | GPU side | same pixels | batched not lower |", "|---|---|---|---|---|---|---|"]
        for r in leg_b(args.images, args.folder_repeats):
            l, b, g = r["loop"], r["batch"], r["gpu_only"]
            verdict = "yes" if b[0] >= l[0] or b[2] >= l[1] else "NO"
            lines.append(f"| {r['dtype']} | {l[0]:.1f} ({l[1]:.1f} .. {l[2]:.1f}) | {b[0]:.1f} ({b[1]:.1f} .. {b[2]:.1f}) | {b[0] / l[0]:.2f}x | "
                         f"{g[0]:.1f} ({g[1]:.1f} .. {g[2]:.1f}) | {'yes' if r['same'] else 'NO'} | {verdict} |")
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
