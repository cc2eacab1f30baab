"""Writes tests/golden/midas_*.npz: inputs, losses and fp32 autograd gradients of the reference's MiDaS loss on the CPU.

    python tools/make_midas_golden.py --omnidata <checkout of EPFL-VILAB/omnidata>

Loads omnidata_tools/torch/losses/midas_loss.py (and the masked_losses.py it imports) from that checkout at run time as a
package; nothing of it is copied here.  Each loss case stores pred, target [B,1,H,W] fp32, mask [B,1,H,W] bool, alpha,
scales, image_based, losses = (total, ssi, reg) and grad = d total / d pred.  midas_parts.npz stores the outputs of
SSIMAE, GradientMatchingTerm (both reductions), compute_scale_and_shift and masked_shift_and_scale on one input.
"""
from __future__ import annotations

import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")


def load_reference(checkout: str):
    pkg_dir = os.path.join(checkout, "omnidata_tools", "torch", "losses")
    spec = importlib.util.spec_from_file_location("reference_losses", os.path.join(pkg_dir, "__init__.py"),
                                                  submodule_search_locations=[pkg_dir])
    pkg = importlib.util.module_from_spec(spec)
    sys.modules["reference_losses"] = pkg
    spec.loader.exec_module(pkg)
    spec = importlib.util.spec_from_file_location("reference_losses.midas_loss", os.path.join(pkg_dir, "midas_loss.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["reference_losses.midas_loss"] = mod
    spec.loader.exec_module(mod)
    return mod


def smooth(rng, B, H, W, lo, hi, k=6):
    """[B,1,H,W] fp32 smooth random field in [lo, hi] (bilinear upsampling of a coarse grid)."""
    g = torch.from_numpy(rng.random((B, 1, k, k)).astype(np.float32))
    f = torch.nn.functional.interpolate(g, size=(H, W), mode="bilinear", align_corners=True)
    f = (f - f.amin((2, 3), keepdim=True)) / (f.amax((2, 3), keepdim=True) - f.amin((2, 3), keepdim=True))
    return (lo + (hi - lo) * f).float().contiguous()


def pair(rng, B, H, W):
    """a target depth and a prediction that differs from it by an affine map, a smooth field and noise"""
    t = smooth(rng, B, H, W, 0.5, 6.0)
    p = 0.7 * t + 0.3 + 0.5 * smooth(rng, B, H, W, 0.0, 1.0) + torch.from_numpy(rng.normal(0, 0.02, t.shape).astype(np.float32))
    return p.float().contiguous(), t


def run(ref, pred, target, mask, alpha=0.1, scales=4, reduction="image-based"):
    p = pred.clone().requires_grad_(True)
    total, ssi, reg = ref.MidasLoss(alpha=alpha, scales=scales, reduction=reduction)(p, target, mask)
    total.backward()
    return dict(pred=pred, target=target, mask=mask, alpha=np.float64(alpha), scales=np.int64(scales),
                image_based=np.int64(reduction != "batch-based"),
                losses=torch.stack([total.detach(), ssi.detach(), torch.as_tensor(reg).detach().float()]), grad=p.grad)


def save(name, d):
    arrs = {k: (v.numpy() if isinstance(v, torch.Tensor) else v) for k, v in d.items()}
    path = os.path.join(OUT, f"midas_{name}.npz")
    np.savez_compressed(path, **arrs)
    print(f"{path}: {os.path.getsize(path)} B")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--omnidata", required=True, help="checkout of the reference repository")
    args = ap.parse_args()
    ref = load_reference(args.omnidata)
    rng = np.random.default_rng(20261016)
    torch.set_num_threads(4)

    # 1. smooth depth, 80 % mask, MidasLoss defaults
    p, t = pair(rng, 3, 48, 64)
    save("smooth", run(ref, p, t, torch.from_numpy(rng.random(p.shape) < 0.8)))
    # 2. batch-based reduction, scales = 3, alpha = 0.5
    p, t = pair(rng, 3, 40, 56)
    save("batch_s3", run(ref, p, t, torch.from_numpy(rng.random(p.shape) < 0.8), alpha=0.5, scales=3, reduction="batch-based"))
    # 3. masks: one empty image, one single-pixel image, one 1 % image
    p, t = pair(rng, 4, 40, 48)
    m = torch.from_numpy(rng.random(p.shape) < 0.8)
    m[1] = False
    m[2] = False
    m[2, 0, 17, 23] = True
    m[3] = torch.from_numpy(rng.random((1, 40, 48)) < 0.01)
    save("masks", run(ref, p, t, m))
    # 4. quantised depths: many ties, in the medians too
    p, t = pair(rng, 2, 40, 48)
    p, t = (p * 4).round() / 4, (t * 2).round() / 2
    save("ties", run(ref, p, t, torch.from_numpy(rng.random(p.shape) < 0.8)))
    # 5. odd sizes
    p, t = pair(rng, 2, 37, 53)
    save("odd", run(ref, p, t, torch.from_numpy(rng.random(p.shape) < 0.8), alpha=0.1, scales=4))
    # 6. the separate callables on one input
    p, t = pair(rng, 2, 33, 45)
    m = torch.from_numpy(rng.random(p.shape) < 0.8)
    pa, ta = ref.masked_shift_and_scale(p, t, m)
    ssi = ref.SSIMAE()(p, t, m)
    sc, sh = ref.compute_scale_and_shift(p[:, 0], t[:, 0], m[:, 0])
    gm_b = ref.GradientMatchingTerm(scales=4, reduction="batch-based")(p[:, 0], t[:, 0], m[:, 0])
    gm_i = ref.GradientMatchingTerm(scales=3, reduction="image-based")(p[:, 0], t[:, 0], m[:, 0])
    save("parts", dict(pred=p, target=t, mask=m, pred_aligned=pa, target_aligned=ta, ssi=ssi.detach(), scale=sc, shift=sh,
                       gm_batch_s4=torch.as_tensor(gm_b).float(), gm_image_s3=torch.as_tensor(gm_i).float()))


if __name__ == "__main__":
    main()
