"""Times the version-1 UNet forward: the engine (omnidata_amd.unet.UNetEngine) against the same network in torch 16-bit ops
(tests/unet_restatement.TorchUNet under .half() / .bfloat16()) on the same GPU, in the same process.

    python tools/unet_bench.py [--batches 1,32] [--hw 384] [--windows 5] [--iters 0] [--md profiles/unet_bench.md]

Per (dtype, batch): after a warm-up of both paths, `windows` alternating windows (engine, torch, engine, ...) of `iters`
forwards each between two HIP events (iters 0: as many as make a window of about 0.3 s); the medians over the windows are
reported as images/s.  Also the engine's time by launch class -- the small-channel convolution kernel (+ the first layer's
im2col), the launch_gemm convolutions, and the GroupNorm / up-sample / head passes -- each timed alone through
dptx_unet_debug_forward_classes (the launches of one class only, on whatever the arena holds: same shapes, same work), and
the largest difference of the two paths' results.  Needs a GPU: there is no CPU fallback.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters   # ms per forward


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,32")
    ap.add_argument("--hw", type=int, default=384)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=0)
    ap.add_argument("--dtypes", default="fp16,bf16")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--md", default=None, help="also write the table as markdown")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("unet_bench.py needs an AMD GPU: nothing is measured without one")
    from omnidata_amd.unet import UNetEngine
    from tests.unet_restatement import TorchUNet, unet_input, unet_random_state_dict

    dev = torch.device("cuda:0")
    sd = unet_random_state_dict(args.seed, 3)
    batches = [int(b) for b in args.batches.split(",")]
    rows = []
    for dtype in args.dtypes.split(","):
        tdt = {"fp16": torch.float16, "bf16": torch.bfloat16}[dtype]
        ref = TorchUNet(sd).to(dev).to(tdt).eval()
        eng = UNetEngine(out_channels=3, max_batch=max(batches), dtype=dtype, device_id=0, max_hw=(args.hw, args.hw))
        eng.load_state_dict(sd)
        for B in batches:
            x = unet_input(args.seed, B, args.hw, args.hw).to(dev)
            xt = x.to(tdt)
            y = torch.empty(B, 3, args.hw, args.hw, device=dev)

            def run_engine(classes=7):
                eng.forward(x, out=y, classes=classes)

            def run_torch():
                with torch.no_grad():
                    return ref(xt)

            for _ in range(3):   # warm-up: code objects, torch's algorithm choices
                run_engine()
                yt = run_torch()
            torch.cuda.synchronize()
            diff = float((y - yt.float()).abs().max())
            iters_e = args.iters or max(3, int(300.0 / max(window(run_engine, 3), 1e-3)))
            iters_t = args.iters or max(3, int(300.0 / max(window(run_torch, 3), 1e-3)))
            te, tt = [], []
            for _ in range(args.windows):
                te.append(window(run_engine, iters_e))
                tt.append(window(run_torch, iters_t))
            cls = {}
            for name, mask in (("small_conv", 1), ("gemm_conv", 2), ("passes", 4)):
                run_engine(mask)
                torch.cuda.synchronize()
                cls[name] = statistics.median(window(lambda: run_engine(mask), iters_e) for _ in range(3))
            run_engine()   # leave a valid result behind
            torch.cuda.synchronize()
            me, mt = statistics.median(te), statistics.median(tt)
            rows.append(dict(dtype=dtype, batch=B, hw=args.hw, engine_ms=me, torch_ms=mt, engine_img_s=B * 1e3 / me,
                             torch_img_s=B * 1e3 / mt, engine_ms_windows=te, torch_ms_windows=tt, class_ms=cls,
                             max_abs_diff_engine_vs_torch16=diff, iters=(iters_e, iters_t)))
            print(json.dumps(rows[-1]))
        eng.close()
        del ref
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)
    if args.md:
        with open(args.md, "w") as f:
            f.write("| dtype | batch | engine images/s | torch 16-bit images/s | engine / torch | engine ms | small-channel convs ms | "
                    "launch_gemm convs ms | norm / resample passes ms |\n|---|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                c = r["class_ms"]
                f.write(f"| {r['dtype']} | {r['batch']} | {r['engine_img_s']:.1f} | {r['torch_img_s']:.1f} | "
                        f"{r['torch_ms'] / r['engine_ms']:.2f} | {r['engine_ms']:.3f} | {c['small_conv']:.3f} | {c['gemm_conv']:.3f} | "
                        f"{c['passes']:.3f} |\n")


if __name__ == "__main__":
    main()
