"""Writes tests/golden/refocus_*.npz: inputs and outputs of the reference's 3D refocus augmentation, run on the CPU.

    python tools/make_refocus_golden.py --omnidata <checkout of EPFL-VILAB/omnidata>

Loads omnidata_tools/torch/data/refocus_augmentation.py from that checkout at run time (nothing of it is copied here),
with two shims: `seaborn` (imported there, never used) is stubbed, and torch.nn.parallel.parallel_apply -- which needs a
GPU even for CPU tensors -- is replaced by the sequential [m(*a) for m, a in zip(modules, args)], which computes the same
thing.  Each case stores the inputs, focus, aperture, quantile_vals [B, n+1], segments and the output.
"""
from __future__ import annotations

import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")


def load_reference(checkout: str):
    path = os.path.join(checkout, "omnidata_tools", "torch", "data", "refocus_augmentation.py")
    sys.modules.setdefault("seaborn", types.ModuleType("seaborn"))
    spec = importlib.util.spec_from_file_location("reference_refocus_augmentation", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.parallel_apply = lambda modules, args: [m(*a) for m, a in zip(modules, args)]
    return mod


def smooth_field(rng, B, H, W, lo, hi, k=6):
    """[B,1,H,W] fp32 smooth random depth in [lo, hi] (bilinear upsampling of a coarse grid)."""
    g = torch.from_numpy(rng.random((B, 1, k, k)).astype(np.float32))
    f = torch.nn.functional.interpolate(g, size=(H, W), mode="bilinear", align_corners=True)
    f = (f - f.amin((2, 3), keepdim=True)) / (f.amax((2, 3), keepdim=True) - f.amin((2, 3), keepdim=True))
    return (lo + (hi - lo) * f).float().contiguous()


def image(rng, B, C, H, W):
    return torch.from_numpy(rng.random((B, C, H, W)).astype(np.float32))


def run_direct(ref, rgb, depth, n, focus_idx, aperture):
    quantiles = torch.arange(0, n + 1) / n
    _, qv = ref.compute_quantiles(depth, quantiles, eps=0.0001)
    qv = qv.permute(1, 0)
    focus = torch.gather(qv, 1, torch.tensor(focus_idx).unsqueeze(1))
    ap = torch.tensor(aperture, dtype=torch.float32).reshape(-1, 1)
    out, seg = ref.refocus_image(rgb, depth, focus, ap, qv, return_segments=True)
    return dict(rgb=rgb, depth=depth, n=np.int64(n), focus=focus, aperture=ap, quantile_vals=qv, segments=seg, out=out)


def save(name, d):
    arrs = {k: (v.numpy() if isinstance(v, torch.Tensor) else v) for k, v in d.items()}
    arrs["segments"] = arrs["segments"].astype(np.int8)  # indices <= n (small): stored narrow, compared as int64
    path = os.path.join(OUT, f"refocus_{name}.npz")
    np.savez_compressed(path, **arrs)
    r = ref_radii(d)
    print(f"{path}: {os.path.getsize(path)} B, radii {r.min():.3g} .. {r.max():.3g}")


def ref_radii(d):
    q, f, a = d["quantile_vals"], d["focus"], d["aperture"]
    return (a * torch.abs(q - f) / q).numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--omnidata", required=True, help="checkout of the reference repository")
    args = ap.parse_args()
    ref = load_reference(args.omnidata)
    rng = np.random.default_rng(20261016)
    torch.set_num_threads(4)

    # 1. B=2, C=3, 48x64, n=10: near quantiles far from focus -> radii up to ~10x the image width (M > 2W)
    depth = smooth_field(rng, 2, 48, 64, 0.05, 3.0)
    save("wide", run_direct(ref, image(rng, 2, 3, 48, 64), depth, 10, [9, 6], [6.0, 0.8]))

    # 2. depth decoded from 16-bit PNG values as the CLI does (v / 65535 / (8000 / 65535)): ties, and a far plateau at 65535
    v = (smooth_field(rng, 2, 40, 56, 300.0, 9000.0) / 64).round() * 64
    v[:, :, :12, :] = 65535.0
    depth = (v / 65535.0) / torch.tensor(8000.0 / 65535.0)
    save("u16_plateau", run_direct(ref, image(rng, 2, 3, 40, 56), depth.float(), 10, [3, 8], [2.5, 5.0]))

    # 3. C=1 at 37x53, n=4
    depth = smooth_field(rng, 1, 37, 53, 0.4, 2.0)
    save("c1_odd", run_direct(ref, image(rng, 1, 1, 37, 53), depth, 4, [2], [1.5]))

    # 4. minimum depth 0: q_0 = -1e-4, a negative radius (no blur)
    depth = smooth_field(rng, 1, 32, 40, 0.0, 1.5)
    save("zero_min", run_direct(ref, image(rng, 1, 3, 32, 40), depth, 6, [3], [3.0]))

    # 5. the reference's own draws: RefocusImageAugmentation(10, 0.001, 6) on the CPU after torch.manual_seed(seed)
    seed = 1234
    rgb, depth = image(rng, 3, 3, 32, 48), smooth_field(rng, 3, 32, 48, 0.2, 4.0)
    seen = {}
    orig = ref.refocus_image

    def spy(rgb_, depth_, focus, aperture, qv, return_segments=False):
        seen.update(focus=focus.clone(), aperture=aperture.clone(), quantile_vals=qv.clone())
        return orig(rgb_, depth_, focus, aperture, qv, return_segments)

    ref.refocus_image = spy
    torch.manual_seed(seed)
    out, seg = ref.RefocusImageAugmentation(10, 0.001, 6, return_segments=True)(rgb, depth)
    ref.refocus_image = orig
    save("seeded", dict(rgb=rgb, depth=depth, n=np.int64(10), seed=np.int64(seed), segments=seg, out=out, **seen))


if __name__ == "__main__":
    main()
